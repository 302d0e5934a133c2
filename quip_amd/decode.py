"""The decode loop of the reference's `benchmark()` (opt.py:431-482, llama.py:418-471) on packed layers.

The reference times `model(input_ids[:, i], past_key_values=...)` token by token on the Hugging Face model whose Linears
were fake-quantised (its packed kernels were never runnable, quant.py:166-169).  Here the same loop runs on the packed
`QuantLinear` layers themselves:

    with decode.collect_packed() as packed:          # QuantMethod.free() hands every quantised Linear over as a QuantLinear
        opt_sequential(model, dataloader, DEV)       # the reference's own driver, unmodified (opt.py:29-190)
    packed.install(model)                            # make_quant: nn.Linear -> QuantLinear inside the HF model
    engine = decode.DecodeEngine.from_hf(model)      # static KV cache, device-resident position, ONE hipGraph per token
    decode.benchmark(model, input_ids, check=True)   # opt.py:431-482's loop and printout

`from_hf` reads the architecture off an `OPTForCausalLM` / `LlamaForCausalLM` (embeddings, norms, head, the block's Linears --
packed or still dense) and picks the fastest launch sequence the layers allow:

    v3_head  5 (OPT) / 6 (Llama) launches per block + 2 per token: csrc/decode_fused.hip, decode_attn.hip, decode_bigp.hip,
             decode_head.hip -- 2-bit qfn-b layers with Kronecker operators (preproc_proj_extra = 1), fp16, <= 4 rows
    fused    three launches per packed layer group (operator / grouped dequant-GEMM / operator), single-launch attention --
             any packed layer; an operator the small-batch kernels cannot take (the blocked butterfly preproc_proj_extra = 0
             yields, a 688 x 16 factor) runs on the general K3 launches for that side only
    plain    layer.forward() per Linear (also dense nn.Linear models: the fp16 baseline of the same harness)

There is no CPU path: the engine raises on a model that is not on a GPU."""
import collections
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import method as _method
from . import ops
from .quant import (QuantLinear, make_quant, packed_forward_fused, fused_stage, fused_ok, fused_attention, fused_attention_ok,
                    fused_u_only, fused_head, fused_head_ok, fused_bigp_tail, bigp_tail_ok, packed_u_stage, stage_operands, attention_operands)

MODES = ("plain", "fused", "v3", "v3_head")
OPERAND_PREFETCH = False   # True: v3 launches carry 8 spare workgroups that pull the step-independent operands of a LATER launch of the block into
                           # every XCD's L2 (csrc/prefetch.h; in a decode step they are cold once per token).  Measured NEUTRAL (profiles/
                           # r06f_decode_ab.jsonl, one box, alternating: OPT-1.3B 1183-1194 tok/s off, 1180-1191 on; Llama-2-7B 610-617 / 618-620;
                           # 4 sequences -2 %): what the warm operands save the consuming launch, the extra workgroups cost the hosting one.  Off.


# ------------------------------------------------------------------------------------------------ packed layers out of a driver run
def _groupwise_unpackable(m):
    """why a method that kept codes beside group tables (GPTQ with --groupsize) cannot become a group-wise QuantLinear, or None when it
    can (also for every method without groups)"""
    gs = getattr(m, 'group_scale', None)
    if gs is None or getattr(m, 'group_zero', None) is None:
        return None
    rows, cols = m.codes.shape
    G = cols // max(gs.shape[1], 1)
    bits = int(torch.log2(m.quantizer.maxq.float() + 1).round().item())
    if G not in ops.GROUPSIZES:
        return f"groupsize {G}: the group-wise dequant-GEMM serves 32, 64 and 128"
    if bits not in (2, 3, 4):
        return f"{bits} bits: packed layers hold 2, 3 or 4"
    if rows % 16 or cols % ops.stream_chunk(bits):
        return f"the STREAM layout needs out_features % 16 == 0 and in_features % {ops.stream_chunk(bits)} == 0"
    return None


class collect_packed:
    """context manager: while it is active every `QuantMethod.free()` (the last call the reference's drivers make on a method,
    opt.py:166, llama.py:150) first turns the method's integer state into a packed `QuantLinear` (QuantLinear.from_method: codes,
    grid, rescale vector, operators -- what the reference throws away, method.py:223-225).  Methods without integer codes
    (Nearest, GPTQ's column walk) are skipped and stay dense.  GPTQ with `--groupsize` 32 / 64 / 128 yields a group-wise QuantLinear (one
    (scale, zero) per row and group, csrc/dqgemm_gw.hip); groups of 16, or a shape the STREAM layout cannot hold, stay dense with one
    printed line.  `install(model)` swaps the collected layers into the model.
    native3: layers quantised to 3 bits are packed in the STREAM3 layout (3 bits per weight) instead of the 4-bit container; ignored
    for every other width."""

    def __init__(self, native3=False):
        self.native3 = native3
        self.layers = []          # [(the nn.Linear that was quantised, its QuantLinear)]

    def __enter__(self):
        self._orig = orig = _method.QuantMethod.free
        got, native3 = self.layers, self.native3

        def free(m):
            if getattr(m, 'codes', None) is not None and isinstance(m.layer, nn.Linear):
                why = _groupwise_unpackable(m)
                if why is None:
                    got.append((m.layer, QuantLinear.from_method(m, m.layer, native3=native3)))
                else:                                     # one line, no exception in the middle of a driver run: the layer stays dense
                    print(f"collect_packed: a {m.codes.shape[0]} x {m.codes.shape[1]} layer quantised with groups stays dense ({why})")
                m.codes = None
            return orig(m)
        _method.QuantMethod.free = free
        return self

    def __exit__(self, *exc):
        _method.QuantMethod.free = self._orig
        return False

    def named(self, model):
        by_id = {id(lin): ql for lin, ql in self.layers}
        return {name: by_id[id(mod)] for name, mod in model.named_modules() if id(mod) in by_id}

    def install(self, model):
        """replace the quantised nn.Linear modules of `model` by their packed layers; returns {dotted name: QuantLinear}"""
        named = self.named(model)
        make_quant(model, named)
        return named


# ------------------------------------------------------------------------------------------------ OPT
def _is_packed(*layers):
    return all(isinstance(l, QuantLinear) for l in layers)


class OPTBlock(nn.Module):
    """one pre-LN OPT decoder layer over given modules (nn.Linear or QuantLinear; HF's OPTDecoderLayer parts)"""

    def __init__(self, ln1, q_proj, k_proj, v_proj, out_proj, ln2, fc1, fc2, heads):
        super().__init__()
        self.ln1, self.ln2 = ln1, ln2
        self.q_proj, self.k_proj, self.v_proj, self.out_proj, self.fc1, self.fc2 = q_proj, k_proj, v_proj, out_proj, fc1, fc2
        self.h = ln1.weight.numel()
        self.heads, self.hd = heads, self.h // heads
        self.fused = False        # packed layers: q/k/v grouped, LayerNorm / residual / ReLU folded into the operator launches
        self.fused_attn = True    # cache append + q K^T + softmax + p V as one launch (csrc/decode_attn.hip)

    @classmethod
    def random(cls, h, ffn, heads, dtype):
        mk = lambda i, o: nn.Linear(i, o, bias=True, dtype=dtype)
        return cls(nn.LayerNorm(h, dtype=dtype), mk(h, h), mk(h, h), mk(h, h), mk(h, h), nn.LayerNorm(h, dtype=dtype), mk(h, ffn), mk(ffn, h), heads)

    def forward(self, x, kc, vc, pos, mask):
        """x [bs, h]; kc / vc [bs, heads, maxlen, hd]; pos int64 [1] on the device; mask [maxlen] additive (eager attention only)."""
        bs = x.shape[0]
        if self.fused:
            q, k, v = packed_forward_fused([self.q_proj, self.k_proj, self.v_proj], x, ln=self.ln1)
        else:
            hn = self.ln1(x)
            q, k, v = self.q_proj(hn), self.k_proj(hn), self.v_proj(hn)
        if self.fused_attn:
            o = ops.decode_attention(q.contiguous(), k.contiguous(), v.contiguous(), kc, vc, pos)
        else:                                               # the eager chain of HF's attention: nine launches
            q, k, v = (t.view(bs, self.heads, 1, self.hd) for t in (q, k, v))
            kc.index_copy_(2, pos, k)
            vc.index_copy_(2, pos, v)
            att = torch.matmul(q, kc.transpose(2, 3)) * (1.0 / self.hd ** 0.5) + mask    # [bs, heads, 1, maxlen]
            att = torch.softmax(att.float(), -1).to(x.dtype)
            o = torch.matmul(att, vc).reshape(bs, self.h)
        if self.fused:
            x = packed_forward_fused([self.out_proj], o, residual=x)[0]
            hmid = packed_forward_fused([self.fc1], x, ln=self.ln2, relu=True)[0]
            return packed_forward_fused([self.fc2], hmid, residual=x)[0]
        x = x + self.out_proj(o)
        x = x + self.fc2(F.relu(self.fc1(self.ln2(x))))
        return x


    def prefill(self, x, kc, vc, start, T):
        """T new positions per sequence in one pass: x [bs*T, h] (row b*T + t), start int64 [1] on the device.  The projections run through
        the layers' own forward (K3 row operators + the batched K2 kernel for packed layers), the attention is ops.prefill_attention."""
        hn = self.ln1(x)
        q, k, v = self.q_proj(hn), self.k_proj(hn), self.v_proj(hn)
        o = ops.prefill_attention(q, k, v, kc, vc, start, T)
        x = x + self.out_proj(o)
        return x + self.fc2(F.relu(self.fc1(self.ln2(x))))


class OPTDecoder(nn.Module):
    """token + learned position embedding (offset 2), the blocks, final LayerNorm, head (tied to the embedding unless given)"""
    arch = "opt"

    def __init__(self, tok, posemb, blocks, lnf, heads, lm_head_weight=None):
        super().__init__()
        self.tok, self.posemb, self.lnf = tok, posemb, lnf
        self.blocks = blocks if isinstance(blocks, nn.ModuleList) else nn.ModuleList(blocks)
        self.h, self.layers_n, self.heads = tok.weight.shape[1], len(self.blocks), heads
        self._head_w = lm_head_weight

    v3 = False               # csrc/decode_fused.hip: everything between two GEMMs in the consuming GEMM's prologue -- 5 launches per block
    v3_attn = True           # with v3: the output-side operators of q / k / v in the attention launch (csrc/decode_attn.hip)
    fused_head = False       # with v3: embedding (+ the previous step's argmax) and [U_fc2^T + residual -> final LN -> lm_head -> argmax
                             # partials, pos += 1] as one launch each (csrc/decode_head.hip)

    @property
    def head_weight(self):
        return self.tok.weight if self._head_w is None else self._head_w

    @property
    def kv_heads(self):
        return self.heads

    def packed(self):
        return all(_is_packed(b.q_proj, b.k_proj, b.v_proj, b.out_proj, b.fc1, b.fc2) for b in self.blocks)

    def v3_ok(self, bs, max_len=None):
        """(max_len: no bound here -- a block whose cache the fused attention launch cannot hold runs ops.decode_attention, blocks_v3)"""
        b = self.blocks[0]
        return (self.packed() and fused_ok([b.q_proj, b.k_proj, b.v_proj], bs, prev=b.fc2) and fused_ok([b.out_proj], bs, norm=False)
                and fused_ok([b.fc1], bs, prev=b.out_proj) and fused_ok([b.fc2], bs, prev=b.fc1, norm=False, residual=False))

    def head_ok(self, bs):
        return fused_head_ok(self.blocks[-1].fc2, bs, self.lnf)

    def embed(self, ids, pos):
        return self.tok(ids) + F.embedding(pos + 2, self.posemb.weight)

    def head(self, x):
        return F.linear(self.lnf(x), self.head_weight)

    def step_v3(self, x, pos, caches):
        prev, y2, x = self.blocks_v3(x, pos, caches)
        return fused_u_only(prev, y2, residual=x)

    def step_fused_head(self, ids, pos, caches, logits, part_val, part_idx):
        x = torch.empty((ids.numel(), self.h), dtype=torch.float16, device=ids.device)
        ops.decode_embed(self.tok.weight, ids, x, pos_table=self.posemb.weight, pos=pos, pos_offset=2, part_val=part_val, part_idx=part_idx)
        prev, y2, x = self.blocks_v3(x, pos, caches)
        return fused_head(prev, y2, x, self.lnf, self.head_weight, logits, part_val, part_idx, pos_inc=pos)

    def _operand_lists(self):
        """per block: the step-independent operand tensors of each of its five launches (quant.stage_operands), built once"""
        pf = self.__dict__.get('_pf_lists')
        if pf is None:
            pf, prev = [], None
            for blk in self.blocks:
                qkv = [blk.q_proj, blk.k_proj, blk.v_proj]
                pf.append({"qkv": stage_operands(qkv, prev=prev, ln=blk.ln1), "attn": attention_operands(qkv), "o": stage_operands([blk.out_proj]),
                           "fc1": stage_operands([blk.fc1], prev=blk.out_proj, ln=blk.ln2), "fc2": stage_operands([blk.fc2], prev=blk.fc1)})
                prev = blk.fc2
            # (the fc1 -> fc2 launch's per-lane tables are built by its first call: keep the lists only once they are in)
            if all(b.fc2.__dict__.get('_pair_tables') or (b.fc2.V.p, b.fc2.V.q) != (128, 64) for b in self.blocks):
                self.__dict__['_pf_lists'] = pf
        return pf

    def blocks_v3(self, x, pos, caches):
        """per block: [U_fc2^T(prev) + residual -> LN1 -> V_qkv -> GEMM qkv] [U_qkv^T + attention] [V_o -> GEMM o]
        [U_o^T + residual -> LN2 -> V_fc1 -> GEMM fc1] [U_fc1^T + relu -> V_fc2 -> GEMM fc2]; returns (fc2 of the last block, its output
        in the projected basis, the residual stream): the last U_fc2^T + residual belongs to whatever ends the step.
        With OPERAND_PREFETCH the qkv launch (192 workgroups on 256 CUs) also pulls the attention launch's operands into the L2s, the
        attention launch (32 workgroups) those of out_proj and fc1, the out_proj launch (64) those of fc2 and of the next block's qkv."""
        dt = x.dtype
        prev, y2 = None, None
        h16 = torch.float16                                     # y consumed by another fused launch: fp16 (its scatter rounds to fp16 anyway)
        pf = self._operand_lists() if OPERAND_PREFETCH else None
        for bi, (blk, (kc, vc)) in enumerate(zip(self.blocks, caches)):
            qkv = [blk.q_proj, blk.k_proj, blk.v_proj]
            attn_u = self.v3_attn and fused_attention_ok(qkv, kc)
            ydt = h16 if attn_u else torch.float32
            if pf is not None and attn_u:
                ops.decode_prefetch_next(pf[bi]["attn"])
            if prev is None:
                ys, _ = fused_stage(qkv, x=x, ln=blk.ln1, y_dtype=ydt)
            else:
                ys, x = fused_stage(qkv, prev=prev, y_prev=y2, residual=x, ln=blk.ln1, store=True, y_dtype=ydt)
            if attn_u:                                          # U_q^T, U_k^T, U_v^T + bias in the attention launch's prologue
                if pf is not None:
                    ops.decode_prefetch_next((pf[bi]["o"] + pf[bi]["fc1"])[:40])
                o = fused_attention(qkv, ys, kc, vc, pos)
            else:                                               # (the fused launches hand y over in ZT order: K3 wants the natural one)
                q, k, v = packed_u_stage(qkv, [l.from_zt(y) for l, y in zip(qkv, ys)], dt)
                o = ops.decode_attention(q, k, v, kc, vc, pos)
            if pf is not None:
                ops.decode_prefetch_next((pf[bi]["fc2"] + (pf[bi + 1]["qkv"] if bi + 1 < len(pf) else []))[:40])
            yo = fused_stage([blk.out_proj], x=o, y_dtype=h16)[0][0]
            (y1,), x = fused_stage([blk.fc1], prev=blk.out_proj, y_prev=yo, residual=x, ln=blk.ln2, store=True, y_dtype=h16)
            y2 = fused_stage([blk.fc2], prev=blk.fc1, y_prev=y1, relu=True, y_dtype=h16)[0][0]
            prev = blk.fc2
        return prev, y2, x

    def prefill(self, ids, pos, caches, arange, all_logits=False, hidden=False):
        """ids int64 [bs, T] at cache positions pos .. pos + T - 1 (pos int64 [1] on the device, not advanced here); returns the logits of
        the last position [bs, vocab], or of every position [bs, T, vocab]; hidden=True: no head -- the final LayerNorm's output of every
        position [bs * T, h], what the head multiplies (DecodeEngine.score hands it to ops.head_score)"""
        bs, T = ids.shape
        x = self.tok(ids) + F.embedding(arange[:T] + pos + 2, self.posemb.weight)        # learned positions start + t + 2
        x = x.reshape(bs * T, self.h)
        for blk, (kc, vc) in zip(self.blocks, caches):
            x = blk.prefill(x, kc, vc, pos, T)
        if hidden:
            return self.lnf(x)
        if all_logits:
            return self.head(x).view(bs, T, -1)
        return self.head(x.view(bs, T, self.h)[:, -1])

    def step(self, ids, pos, caches, arange):
        """one token for every batch row: ids int64 [bs], pos int64 [1]; returns logits [bs, vocab]."""
        x = self.embed(ids, pos)
        if self.v3:
            return self.head(self.step_v3(x, pos, caches))
        mask = None
        if not all(b.fused_attn for b in self.blocks):
            mask = torch.where(arange <= pos, 0.0, float("-inf")).to(x.dtype)
        for blk, (kc, vc) in zip(self.blocks, caches):
            x = blk(x, kc, vc, pos, mask)
        return self.head(x)


# ------------------------------------------------------------------------------------------------ Llama
class RMSNorm(nn.Module):
    def __init__(self, h, eps, dtype):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(h, dtype=dtype))
        self.eps = eps

    def forward(self, x):                                   # HF LlamaRMSNorm: fp32 statistics, cast, then the gain
        xf = x.float()
        return self.weight * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps)).to(x.dtype)


class LlamaBlock(nn.Module):
    def __init__(self, n1, q_proj, k_proj, v_proj, o_proj, n2, gate_proj, up_proj, down_proj, heads, kv_heads=None):
        super().__init__()
        self.n1, self.n2 = n1, n2
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = q_proj, k_proj, v_proj, o_proj
        self.gate_proj, self.up_proj, self.down_proj = gate_proj, up_proj, down_proj
        self.h = n1.weight.numel()
        self.heads, self.hd = heads, self.h // heads
        self.kv_heads = kv_heads or heads          # < heads: grouped-query attention (k / v have kv_heads * hd outputs)
        self.fused = False

    @classmethod
    def random(cls, h, ffn, heads, eps, dtype, kv_heads=None):
        mk = lambda i, o: nn.Linear(i, o, bias=False, dtype=dtype)
        kv = (kv_heads or heads) * (h // heads)
        return cls(RMSNorm(h, eps, dtype), mk(h, h), mk(h, kv), mk(h, kv), mk(h, h), RMSNorm(h, eps, dtype), mk(h, ffn), mk(h, ffn), mk(ffn, h), heads,
                   kv_heads)

    def forward(self, x, kc, vc, pos, cos, sin, workspace=None):
        """x [bs, h]; kc / vc [bs, kv_heads, maxlen, hd]; pos int64 [1] on the device; cos / sin fp32 [maxpos, hd];
        workspace: ops.decode_attention_grouped_workspace for the caches' shape (grouped-query blocks)."""
        if self.fused:
            q, k, v = packed_forward_fused([self.q_proj, self.k_proj, self.v_proj], x, ln=self.n1)
        else:
            hn = self.n1(x)
            q, k, v = self.q_proj(hn), self.k_proj(hn), self.v_proj(hn)
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if self.kv_heads < self.heads:                      # rotary + append + attention in one launch (csrc/decode_gqa.hip)
            o = ops.decode_attention_grouped(q, k, v, kc, vc, pos, cos, sin, workspace=workspace)
        else:
            ops.rope_inplace(q, k, cos, sin, pos, self.heads)
            o = ops.decode_attention(q, k, v, kc, vc, pos)
        if self.fused:
            x = packed_forward_fused([self.o_proj], o, residual=x)[0]
            g, u = packed_forward_fused([self.gate_proj, self.up_proj], x, ln=self.n2)
            return packed_forward_fused([self.down_proj], g, residual=x, gate_up=u)[0]       # silu(g) * u formed inside the V launch
        x = x + self.o_proj(o)
        hn = self.n2(x)
        return x + self.down_proj(F.silu(self.gate_proj(hn)) * self.up_proj(hn))


    def prefill(self, x, kc, vc, start, T, cos, sin):
        """T new positions per sequence in one pass: x [bs*T, h] (row b*T + t), start int64 [1] on the device; rotary, cache append and
        causal attention are ops.prefill_attention (multi-head and grouped-query alike)"""
        hn = self.n1(x)
        q, k, v = self.q_proj(hn), self.k_proj(hn), self.v_proj(hn)
        o = ops.prefill_attention(q, k, v, kc, vc, start, T, cos, sin)
        x = x + self.o_proj(o)
        hn = self.n2(x)
        return x + self.down_proj(F.silu(self.gate_proj(hn)) * self.up_proj(hn))


def rotary_tables(inv_freq, maxpos):
    """HF LlamaRotaryEmbedding's cos / sin in its duplicated-halves layout, fp32 [maxpos, hd]"""
    fr = torch.outer(torch.arange(maxpos, dtype=torch.float32), inv_freq.float().cpu())
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().contiguous(), emb.sin().contiguous()


class LlamaDecoder(nn.Module):
    arch = "llama"
    NAMES = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]

    def __init__(self, tok, blocks, norm, lm_head, heads, inv_freq, maxpos):
        super().__init__()
        self.tok, self.norm, self.lm_head = tok, norm, lm_head
        self.blocks = blocks if isinstance(blocks, nn.ModuleList) else nn.ModuleList(blocks)
        self.h, self.layers_n, self.heads = tok.weight.shape[1], len(self.blocks), heads
        cos, sin = rotary_tables(inv_freq, maxpos)
        self.register_buffer("cos", cos, persistent=False)
        self.register_buffer("sin", sin, persistent=False)

    def _apply(self, fn, recurse=True):                     # .to(dev) / .half() must not narrow the rotary tables
        cos, sin = self.cos, self.sin
        super()._apply(fn, recurse)
        self.cos, self.sin = cos.to(self.tok.weight.device), sin.to(self.tok.weight.device)
        return self

    v3 = False               # csrc/decode_fused.hip + decode_attn.hip + decode_bigp.hip: 6 launches per block
    fused_head = False       # with v3: embedding (+ the previous step's argmax) and [U_down^T + residual -> final RMSNorm -> lm_head -> argmax
                             # partials, pos += 1] as one launch each (csrc/decode_head.hip)

    attn_workspace = None    # grouped-query blocks: the engine's ops.decode_attention_grouped_workspace (set by DecodeEngine per step)

    @property
    def head_weight(self):
        return self.lm_head.weight

    @property
    def kv_heads(self):
        return self.blocks[0].kv_heads if len(self.blocks) else self.heads

    def packed(self):
        return all(_is_packed(*(getattr(b, n) for n in self.NAMES)) for b in self.blocks)

    def v3_ok(self, bs, max_len=None):
        """can mode v3 run `bs` sequences over KV caches of max_len positions (default: the rotary tables' rows)?  blocks_v3 has no other
        attention than the fused launch, whose LDS bounds the cache (ops.decode_attention_fused_max_len)."""
        b = self.blocks[0]
        qkv = [b.q_proj, b.k_proj, b.v_proj]
        max_len = self.cos.shape[0] if max_len is None else max_len
        return (self.packed() and fused_ok(qkv, bs, prev=b.down_proj) and fused_ok([b.o_proj], bs, norm=False)
                and fused_ok([b.gate_proj, b.up_proj], bs, prev=b.o_proj) and b.down_proj.U is not None and b.down_proj.U.fused_ok
                and bigp_tail_ok([b.gate_proj, b.up_proj], b.down_proj, bs)
                and fused_attention_ok(qkv, torch.empty((bs, self.heads, max_len, b.hd), dtype=torch.float16, device='meta')))

    def head_ok(self, bs):
        return fused_head_ok(self.blocks[-1].down_proj, bs, self.norm)

    def embed(self, ids, pos):
        return self.tok(ids)

    def head(self, x):
        return F.linear(self.norm(x), self.head_weight)

    def step_v3(self, x, pos, caches):
        prev, yd, x = self.blocks_v3(x, pos, caches)
        return fused_u_only(prev, yd.to(torch.float16), residual=x)

    def step_fused_head(self, ids, pos, caches, logits, part_val, part_idx):
        x = torch.empty((ids.numel(), self.h), dtype=torch.float16, device=ids.device)
        ops.decode_embed(self.tok.weight, ids, x, part_val=part_val, part_idx=part_idx)
        prev, yd, x = self.blocks_v3(x, pos, caches)
        return fused_head(prev, yd, x, self.norm, self.head_weight, logits, part_val, part_idx, pos_inc=pos)

    def _operand_lists(self):
        """per block: the step-independent operand tensors of the attention, o_proj and gate / up launches (quant.stage_operands), built once"""
        pf = self.__dict__.get('_pf_lists')
        if pf is None:
            pf = [{"attn": attention_operands([b.q_proj, b.k_proj, b.v_proj]), "o": stage_operands([b.o_proj]),
                   "gu": stage_operands([b.gate_proj, b.up_proj], prev=b.o_proj, ln=b.n2)} for b in self.blocks]
            self.__dict__['_pf_lists'] = pf
        return pf

    def blocks_v3(self, x, pos, caches):
        """per block, six launches: [U_down^T(prev) + residual -> RMSNorm -> V_qkv -> GEMM q,k,v] [U_qkv^T + rotary + attention]
        [V_o -> GEMM o] [U_o^T + residual -> RMSNorm -> V_gate/up -> GEMM gate, up] [U_gate^T, U_up^T (/) s: 688 x 16, decode_bigp.hip]
        [silu * up -> V_down -> GEMM down, K-slices through fp32 atomics]; a 688 x 688 factor is 0.9 MB, not a workgroup's pass: the
        11008-wide operators are cut over the p index (csrc/decode_bigp.hip)"""
        h16 = torch.float16
        prev, yd = None, None
        pf = self._operand_lists() if OPERAND_PREFETCH else None
        for bi, (blk, (kc, vc)) in enumerate(zip(self.blocks, caches)):
            qkv = [blk.q_proj, blk.k_proj, blk.v_proj]
            if pf is not None:                                      # (the q / k / v launch is 192 workgroups: 64 CUs are free for the 8 extra ones)
                ops.decode_prefetch_next(pf[bi]["attn"])
            if prev is None:
                ys, _ = fused_stage(qkv, x=x, ln=blk.n1, y_dtype=h16)
            else:
                ys, x = fused_stage(qkv, prev=prev, y_prev=yd, residual=x, ln=blk.n1, store=True, y_dtype=h16)
            if pf is not None:                                      # the attention launch (32 workgroups): operands of o_proj and of gate / up
                ops.decode_prefetch_next((pf[bi]["o"] + pf[bi]["gu"])[:40])
            o = fused_attention(qkv, ys, kc, vc, pos, self.cos, self.sin)
            yo = fused_stage([blk.o_proj], x=o, y_dtype=h16)[0][0]
            gu = [blk.gate_proj, blk.up_proj]
            ygu, x = fused_stage(gu, prev=blk.o_proj, y_prev=yo, residual=x, ln=blk.n2, store=True, y_dtype=h16)
            yd = fused_bigp_tail(gu, blk.down_proj, ygu)                       # fp32 accumulator, ZT order of down_proj's U
            prev = blk.down_proj
        return prev, yd, x

    def prefill(self, ids, pos, caches, arange, all_logits=False, hidden=False):
        """ids int64 [bs, T] at cache positions pos .. pos + T - 1 (pos int64 [1] on the device, not advanced here); returns the logits of
        the last position [bs, vocab], or of every position [bs, T, vocab]; hidden=True: no head -- the final RMSNorm's output of every
        position [bs * T, h], what the head multiplies (DecodeEngine.score hands it to ops.head_score)"""
        bs, T = ids.shape
        x = self.tok(ids).reshape(bs * T, self.h)
        for blk, (kc, vc) in zip(self.blocks, caches):
            x = blk.prefill(x, kc, vc, pos, T, self.cos, self.sin)
        if hidden:
            return self.norm(x)
        if all_logits:
            return self.head(x).view(bs, T, -1)
        return self.head(x.view(bs, T, self.h)[:, -1])

    def step(self, ids, pos, caches, arange):
        x = self.embed(ids, pos)
        if self.v3:
            return self.head(self.step_v3(x, pos, caches))
        for blk, (kc, vc) in zip(self.blocks, caches):
            x = blk(x, kc, vc, pos, self.cos, self.sin, self.attn_workspace)
        return self.head(x)


# ------------------------------------------------------------------------------------------------ Hugging Face binding
def decoder_from_hf(model, max_len=2048):
    """OPTDecoder / LlamaDecoder over the modules of a Hugging Face `OPTForCausalLM` / `LlamaForCausalLM` (shared, not copied): the
    decoder Linears may be nn.Linear or the QuantLinear layers `make_quant` / `collect_packed.install` put there."""
    cfg = model.config
    mt = getattr(cfg, "model_type", None)
    if mt == "opt":
        d = model.model.decoder
        if not cfg.do_layer_norm_before or getattr(d, "project_in", None) is not None or getattr(d, "project_out", None) is not None:
            raise NotImplementedError("post-LN / projected-embedding OPT variants (opt-350m) are not served by the decode engine")
        if cfg.activation_function != "relu" or d.final_layer_norm is None:
            raise NotImplementedError("OPT decode engine: ReLU feed-forward and a final LayerNorm are assumed")
        heads = cfg.num_attention_heads
        blocks = [OPTBlock(l.self_attn_layer_norm, l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.out_proj,
                           l.final_layer_norm, l.fc1, l.fc2, heads) for l in d.layers]
        tied = model.lm_head.weight.data_ptr() == d.embed_tokens.weight.data_ptr()
        return OPTDecoder(d.embed_tokens, d.embed_positions, blocks, d.final_layer_norm, heads, None if tied else model.lm_head.weight)
    if mt == "llama":
        m = model.model
        heads = cfg.num_attention_heads
        kv_heads = getattr(cfg, "num_key_value_heads", None) or heads
        if cfg.hidden_act != "silu" or getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False):
            raise NotImplementedError("Llama decode engine: SiLU gate, no biases")
        hd = getattr(cfg, "head_dim", None) or cfg.hidden_size // heads
        if hd * heads != cfg.hidden_size:
            raise NotImplementedError("head_dim * heads != hidden_size")
        if kv_heads != heads:                           # grouped-query attention: csrc/decode_gqa.hip's shapes
            g = heads // kv_heads
            if heads % kv_heads or not 2 <= g <= 16 or hd not in (64, 128):
                raise NotImplementedError(f"grouped-query attention with {heads} heads over {kv_heads} key / value heads of dim {hd} "
                                          "(served: heads / kv_heads in 2..16, head_dim 64 or 128)")
        rot = m.rotary_emb
        if float(getattr(rot, "attention_scaling", 1.0)) != 1.0:
            raise NotImplementedError("scaled rotary embeddings")
        blocks = [LlamaBlock(l.input_layernorm, l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.o_proj,
                             l.post_attention_layernorm, l.mlp.gate_proj, l.mlp.up_proj, l.mlp.down_proj, heads, kv_heads) for l in m.layers]
        return LlamaDecoder(m.embed_tokens, blocks, m.norm, model.lm_head, heads, rot.inv_freq, max_len)
    raise NotImplementedError(f"decode engine: model_type {mt!r} (the reference drives OPT and Llama)")


def set_mode(dec, mode):
    """apply one of MODES to a decoder's flags"""
    assert mode in MODES, mode
    for b in dec.blocks:
        b.fused = mode == "fused"
        if hasattr(b, "fused_attn"):
            b.fused_attn = True
    dec.v3 = mode in ("v3", "v3_head")
    dec.fused_head = mode == "v3_head"
    dec.mode = mode


def groupwise_layers(dec):
    """[(dotted name, layer)] of the decoder's group-wise packed layers: they run through their own forward (modes plain / fused), never
    through the fused decode launches, which read one scale per tensor"""
    return [(n, l) for n, l in dec.named_modules() if isinstance(l, QuantLinear) and l.groupwise]


def best_mode(dec, bs, dtype, max_len=None):
    """the fastest launch sequence the decoder's layers allow (module docstring) for `bs` sequences over caches of max_len positions"""
    if dec.packed():
        if groupwise_layers(dec):
            return "fused"
        if dtype == torch.float16 and dec.v3_ok(bs, max_len):
            return "v3_head" if dec.head_ok(bs) else "v3"
        return "fused"
    return "plain"


class Sampling:
    """how DecodeEngine picks a token: temperature, top-k and top-p (Hugging Face's TopKLogitsWarper, then TopPLogitsWarper) and the 64-bit
    seed of the draws -- ops.sample_rows has the arithmetic.  temperature 0 or top_k 1 is greedy.  A plain value: validated here, compared by
    value, no GPU involved.  Stop tokens, the repetition penalty and per-sequence parameters are `Generation`'s.  Not served: min-length,
    frequency / presence penalties, stop strings, beam search."""
    __slots__ = ("temperature", "top_k", "top_p", "seed")

    def __init__(self, temperature=1.0, top_k=0, top_p=1.0, seed=0):
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        try:
            t, p = float(temperature), float(top_p)
        except (TypeError, ValueError):
            raise ValueError(f"Sampling: temperature and top_p must be numbers (got {temperature!r}, {top_p!r})") from None
        if not t >= 0.0 or t == float("inf"):
            raise ValueError(f"Sampling: temperature must be a finite number >= 0 (0: greedy), got {temperature!r}")
        if not 0.0 < p <= 1.0:
            raise ValueError(f"Sampling: top_p must lie in (0, 1] (1: off), got {top_p!r}")
        if not is_int(top_k) or top_k < 0:
            raise ValueError(f"Sampling: top_k must be an integer >= 0 (0: off), got {top_k!r}")
        if not is_int(seed) or not 0 <= seed < 1 << 64:
            raise ValueError(f"Sampling: seed must be an integer in [0, 2^64), got {seed!r}")
        for name, v in zip(self.__slots__, (t, int(top_k), p, int(seed))):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("Sampling is immutable: build a new one")

    def _key(self):
        return (self.temperature, self.top_k, self.top_p, self.seed)

    def __eq__(self, other):
        return isinstance(other, Sampling) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"Sampling(temperature={self.temperature}, top_k={self.top_k}, top_p={self.top_p}, seed={self.seed})"


class Generation:
    """what ends and shapes a DecodeEngine continuation besides the draw itself -- ops.generate_rows has the arithmetic:
      sampling            None (greedy), a `Sampling`, or a sequence of them, one per sequence of the batch
      repetition_penalty  Hugging Face's RepetitionPenaltyLogitsProcessor over every token the sequence holds so far, prompt included:
                          a finite number > 0 (1: off), or a sequence of them, one per sequence of the batch
      stop_ids            at most 16 token ids; a sequence that draws one of them is finished: the stop token is its last, `pad_id` follows
      pad_id              what a finished sequence yields (and is fed) from then on
    A plain value like `Sampling`: validated here, compared by value, no GPU involved; per-sequence lengths are held against the engine's bs
    by rows(bs).  Not served: min-length, frequency / presence penalties, stop strings, beam search."""
    __slots__ = ("sampling", "repetition_penalty", "stop_ids", "pad_id")
    MAX_STOP = ops.GENERATE_MAX_STOP

    def __init__(self, sampling=None, repetition_penalty=1.0, stop_ids=(), pad_id=0):
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        is_seq = lambda v: isinstance(v, (list, tuple))
        if is_seq(sampling):
            sampling = tuple(sampling)
            if not sampling or not all(isinstance(x, Sampling) for x in sampling):
                raise ValueError("Generation: sampling must be None, a Sampling, or a non-empty sequence of Sampling (one per sequence)")
        elif sampling is not None and not isinstance(sampling, Sampling):
            raise ValueError(f"Generation: sampling must be None, a Sampling, or a sequence of Sampling (got {type(sampling).__name__})")

        def penalty(v):
            try:
                f = float(v)
            except (TypeError, ValueError):
                f = float("nan")
            if isinstance(v, bool) or not 0.0 < f < float("inf"):
                raise ValueError(f"Generation: repetition_penalty must be a finite number > 0 (1: off), got {v!r}")
            return f
        if is_seq(repetition_penalty):
            if not repetition_penalty:
                raise ValueError("Generation: repetition_penalty must be a number or a non-empty sequence of numbers (one per sequence)")
            repetition_penalty = tuple(penalty(v) for v in repetition_penalty)
        else:
            repetition_penalty = penalty(repetition_penalty)
        if isinstance(sampling, tuple) and isinstance(repetition_penalty, tuple) and len(sampling) != len(repetition_penalty):
            raise ValueError(f"Generation: {len(sampling)} Sampling values but {len(repetition_penalty)} repetition penalties")
        try:
            stop_ids = tuple(stop_ids)
        except TypeError:
            raise ValueError(f"Generation: stop_ids must be a sequence of token ids (got {stop_ids!r})") from None
        if len(stop_ids) > self.MAX_STOP:
            raise ValueError(f"Generation: at most {self.MAX_STOP} stop ids (got {len(stop_ids)})")
        if not all(is_int(v) and 0 <= v < 1 << 31 for v in stop_ids):
            raise ValueError(f"Generation: stop_ids must be integers in [0, 2^31), got {stop_ids!r}")
        if not is_int(pad_id) or not 0 <= pad_id < 1 << 31:
            raise ValueError(f"Generation: pad_id must be an integer in [0, 2^31), got {pad_id!r}")
        for name, v in zip(self.__slots__, (sampling, repetition_penalty, tuple(int(v) for v in stop_ids), int(pad_id))):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("Generation is immutable: build a new one")

    def rows(self, bs):
        """[(temperature, top_k, top_p, seed, repetition_penalty)] for the bs sequences of an engine; ValueError when a per-sequence setting
        is not bs long"""
        for name in ("sampling", "repetition_penalty"):
            v = getattr(self, name)
            if isinstance(v, tuple) and len(v) != bs:
                raise ValueError(f"Generation: {name} holds {len(v)} values, the engine runs {bs} sequences")
        greedy = Sampling(temperature=0.0)
        out = []
        for b in range(bs):
            s = self.sampling[b] if isinstance(self.sampling, tuple) else self.sampling or greedy
            p = self.repetition_penalty[b] if isinstance(self.repetition_penalty, tuple) else self.repetition_penalty
            out.append((s.temperature, s.top_k, s.top_p, s.seed, p))
        return out

    def _key(self):
        return (self.sampling, self.repetition_penalty, self.stop_ids, self.pad_id)

    def __eq__(self, other):
        return isinstance(other, Generation) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return (f"Generation(sampling={self.sampling!r}, repetition_penalty={self.repetition_penalty}, stop_ids={self.stop_ids}, "
                f"pad_id={self.pad_id})")


class DecodeEngine:
    """benchmark()'s per-token loop as ONE hipGraph replay per token: static KV cache [bs, kv_heads, max_len, hd] per block, position and
    current token on the device.  `forward(ids)` is `model(ids, past_key_values=...)` for the next position; `generate` is greedy unless a
    `Sampling` is set (set_sampling, or generate's `sampling=`): then every step ends with one sample launch (ops.sample_rows) instead of
    the argmax, replayed from a second graph.  The draw for the token fed at cache position t of sequence b is Philox(seed; t, b): the same
    seed gives the same tokens with or without the graph, after prefill() or token-by-token feeding, and again after reset().
    With a `Generation` set (set_generation, or generate's `generation=`) the launch that ends a step is ops.generate_rows instead: per-sequence
    sampling parameters, a repetition penalty over `history`, stop tokens -- a third graph.  An engine that never sets one runs exactly the
    launches and graphs it ran before Generation existed.  Not served: min-length, frequency / presence penalties, stop strings, beam search."""
    poll = 8                 # generate() under a Generation reads `finished` every `poll` steps and stops once every sequence is done; 0: never

    def __init__(self, decoder, bs=1, max_len=2048, mode="auto", graph=True):
        self.dec = decoder
        w = decoder.tok.weight
        if not w.is_cuda:
            raise RuntimeError("DecodeEngine needs the model on a GPU (there is no CPU path)")
        if getattr(decoder, "arch", None) == "opt":       # learned positions: the table (offset 2) bounds the sequence
            max_len = min(max_len, decoder.posemb.weight.shape[0] - 2)
        elif getattr(decoder, "arch", None) == "llama":
            max_len = min(max_len, decoder.cos.shape[0])
        self.dev, self.dtype, self.bs, self.max_len = w.device, w.dtype, bs, max_len
        self.mode = best_mode(decoder, bs, self.dtype, max_len) if mode == "auto" else mode
        if self.mode in ("v3", "v3_head"):
            gw = groupwise_layers(decoder)
            if gw:
                raise ValueError(f"DecodeEngine: mode {self.mode!r} runs the fused decode launches, which read one scale per tensor, but layer "
                                 f"{gw[0][0]!r} holds a group-wise grid (groupsize {gw[0][1].groupsize}); use mode 'auto', 'fused' or 'plain'")
        set_mode(decoder, self.mode)
        hd = decoder.h // decoder.heads
        kv_heads = decoder.kv_heads
        z = lambda: torch.zeros(bs, kv_heads, max_len, hd, dtype=self.dtype, device=self.dev)
        self.caches = [(z(), z()) for _ in range(decoder.layers_n)]
        # grouped-query attention: one workspace for every block's launch (they run one after another), allocated here, never per step
        self.attn_workspace = (ops.decode_attention_grouped_workspace(bs, decoder.heads, kv_heads, hd, max_len, self.dev)
                               if kv_heads < decoder.heads else None)
        self.arange = torch.arange(max_len, device=self.dev)
        self.ids = torch.zeros(bs, dtype=torch.int64, device=self.dev)
        self.pos = torch.zeros(1, dtype=torch.int64, device=self.dev)
        vocab = decoder.head_weight.shape[0]
        self.logits = torch.zeros(bs, vocab, dtype=self.dtype, device=self.dev)
        self._fh = self.mode == "v3_head"
        if self._fh:     # the token comes out of the head launch's partials at the start of the next step; index -1 = "none": the step reads `ids`
            self.part_val = torch.full((bs, ops.HEAD_PARTS), float("-inf"), dtype=torch.float32, device=self.dev)
            self.part_idx = torch.full((bs, ops.HEAD_PARTS), -1, dtype=torch.int32, device=self.dev)
        self._graph = None
        self._want_graph = graph
        self._steps = 0
        self._sampling = None            # None: greedy -- the launch sequence of _one() below, untouched by anything sampling adds
        self._sample_params = None       # the device struct of the sample launch (ops.sample_params), made by the first set_sampling(Sampling)
        self._graph_sampled = None       # the sampled step's graph, captured by the first sampled step
        self._sampling_written = None    # what the device struct holds
        self.logprob = torch.zeros(bs, dtype=torch.float32, device=self.dev)     # log-probability of the token of the last sampled step
        self.kept_n = torch.zeros(bs, dtype=torch.int32, device=self.dev)        # ... how many entries survived top-k / top-p in that step,
        self.kept_mass = torch.ones(bs, dtype=torch.float32, device=self.dev)    # ... and their share of the top-k mass
        self._generation = None          # None: the steps above.  A Generation: every step ends with ops.generate_rows (_one_generation)
        self._generation_written = None  # what the device parameters hold
        self._gen_params = self._stop_ids = None     # ops.generate_params(bs) and int32 [16] stop ids (-1: unused), made by the first set_generation
        self._graphs_generation = {}     # pad_id -> graph (pad_id is an argument of the launch; everything else is read from the device)
        self.history = self.finished = self.stop_pos = None      # int32 [bs, max_len + 1] (-1: not recorded), int32 [bs], int64 [bs] (-1: none)
        self.lengths = None              # after generate() under a Generation: int64 [bs] on the host, tokens up to and including the stop token

    @classmethod
    def from_hf(cls, model, packed=None, bs=1, max_len=2048, mode="auto", graph=True, device=None):
        """engine over a Hugging Face causal LM; `packed` ({dotted name: QuantLinear}, e.g. quant.load_packed(...)) is swapped in first.
        Parts of the model still on the CPU (the reference's drivers park blocks there, llama.py:162) are moved to `device`."""
        if packed:
            make_quant(model, packed)
        dec = decoder_from_hf(model, max_len=max_len)
        if device is None:
            qls = [m for m in model.modules() if isinstance(m, QuantLinear)]
            device = qls[0].qweight.device if qls else next(model.parameters()).device
        dec.to(device)
        return cls(dec, bs=bs, max_len=max_len, mode=mode, graph=graph)

    # -- one step ---------------------------------------------------------------------------------
    @property
    def sampling(self):
        return self._sampling

    def set_sampling(self, sampling):
        """None: greedy (the default).  A `Sampling`: every following step, and the end of prefill(), draws its token with these parameters.
        The parameters live in one device struct that the sample launch reads at run time: changing them rewrites the struct (one small copy)
        and never recaptures the sampled graph."""
        if sampling is not None and not isinstance(sampling, Sampling):
            raise TypeError(f"DecodeEngine.set_sampling: a decode.Sampling or None (got {type(sampling).__name__})")
        if sampling is not None:
            args = (sampling.temperature, sampling.top_k, sampling.top_p, sampling.seed)
            if self._sample_params is None:
                self._sample_params = ops.sample_params(*args, device=self.dev)
            elif sampling != self._sampling_written:
                ops.write_sample_params(self._sample_params, *args)
            self._sampling_written = sampling
        self._sampling = sampling

    def _sample(self):
        """the sample launch: counter = the device position, which by now is the cache position the drawn token will be fed at"""
        ops.sample_rows(self.logits, self._sample_params, self.pos, out=self.ids, logprob=self.logprob, kept_n=self.kept_n, kept_mass=self.kept_mass,
                        clear=self.part_idx if self._fh else None)

    @property
    def generation(self):
        return self._generation

    def set_generation(self, generation):
        """None: the engine as it is without generation control (greedy, or the `Sampling` in force).  A `Generation`: every following step,
        and the end of prefill(), ends with ops.generate_rows.  The first call allocates `history`, `finished` and `stop_pos`; parameters and
        stop ids live on the device and are read by the launch at run time, so changing them rewrites them (two small copies) and never
        recaptures a graph (a new pad_id, an argument of the launch, captures a graph of its own on its first step).  `finished` and
        `stop_pos` are cleared by reset(), not here; `history` records the tokens fed while a Generation is in force.  With stop ids set,
        feed a prompt through prefill(): forward() ends every fed token with a launch, whose token may finish the sequence."""
        if generation is not None and not isinstance(generation, Generation):
            raise TypeError(f"DecodeEngine.set_generation: a decode.Generation or None (got {type(generation).__name__})")
        if generation is not None and generation != self._generation_written:
            rows = generation.rows(self.bs)                                   # raises before anything is written
            stops = list(generation.stop_ids) + [-1] * (Generation.MAX_STOP - len(generation.stop_ids))
            if self._gen_params is None:
                self._gen_params = ops.generate_params(self.bs, device=self.dev)
                self._stop_ids = torch.full((Generation.MAX_STOP,), -1, dtype=torch.int32, device=self.dev)
                self.history = torch.full((self.bs, self.max_len + 1), -1, dtype=torch.int32, device=self.dev)
                self.finished = torch.zeros(self.bs, dtype=torch.int32, device=self.dev)
                self.stop_pos = torch.full((self.bs,), -1, dtype=torch.int64, device=self.dev)
            ops.write_generate_params(self._gen_params, None, *[[r[i] for r in rows] for i in range(5)])
            self._stop_ids.copy_(torch.tensor(stops, dtype=torch.int32))
            self._generation_written = generation
        self._generation = generation

    def _generate_launch(self, fed):
        """the launch that ends a step under a Generation; counter = the device position, as in _sample().  fed: the token just fed at
        position counter - 1 (`ids`, which the launch then overwrites), or None when the caller wrote `history` itself (prefill)"""
        ops.generate_rows(self.logits, self._gen_params, self.pos, hist=self.history, fed=fed, stop_ids=self._stop_ids,
                          pad_id=self._generation.pad_id, done=self.finished, stop_pos=self.stop_pos, out=self.ids, logprob=self.logprob,
                          kept_n=self.kept_n, kept_mass=self.kept_mass, clear=self.part_idx if self._fh else None)

    def _one_generation(self):
        """_one_sampled()'s launch sequence with ops.generate_rows in place of the sample launch, for greedy rows too"""
        if self.attn_workspace is not None:
            self.dec.attn_workspace = self.attn_workspace
        if self._fh:
            self.dec.step_fused_head(self.ids, self.pos, self.caches, self.logits, self.part_val, self.part_idx)
            self._generate_launch(self.ids)
            return
        lg = self.dec.step(self.ids, self.pos, self.caches, self.arange)
        self.logits.copy_(lg)
        self.pos.add_(1)
        self._generate_launch(self.ids)

    def _one_sampled(self):
        if self.attn_workspace is not None:
            self.dec.attn_workspace = self.attn_workspace
        if self._fh:                                     # the head launch wrote fp16 `logits` and advanced pos; clearing its argmax partials makes
            self.dec.step_fused_head(self.ids, self.pos, self.caches, self.logits, self.part_val, self.part_idx)     # the next embed launch read `ids`
            self._sample()
            return
        lg = self.dec.step(self.ids, self.pos, self.caches, self.arange)
        self.logits.copy_(lg)
        self.pos.add_(1)
        self._sample()

    def _one(self):
        if self._generation is not None:
            return self._one_generation()
        if self._sampling is not None:
            return self._one_sampled()
        if self.attn_workspace is not None:              # (a decoder may serve several engines: each step brings its own)
            self.dec.attn_workspace = self.attn_workspace
        if self._fh:
            self.dec.step_fused_head(self.ids, self.pos, self.caches, self.logits, self.part_val, self.part_idx)
            return
        lg = self.dec.step(self.ids, self.pos, self.caches, self.arange)
        self.logits.copy_(lg)
        ops.argmax_rows(lg, out=self.ids)                # one launch (6 us kernel); torch's generic reduction: 18 us for 50272 logits
        self.pos.add_(1)

    def reset(self):
        self.pos.zero_()
        self._steps = 0
        if self._fh:
            self.part_idx.fill_(-1)
        if self.history is not None:
            self.history.fill_(-1)
            self.finished.zero_()
            self.stop_pos.fill_(-1)

    def _state(self):
        ts = [self.pos, self.ids, self.logits, self.logprob]
        if self._generation is not None:                 # ... and what a generate launch at the current position writes besides
            ts += [self.finished, self.stop_pos, self.history[:, self._steps:self._steps + 2]]
        return ts + [self.part_val, self.part_idx] if self._fh else ts

    @torch.no_grad()
    def _capture_in_place(self):
        """capture _one() as it stands at the engine's CURRENT position: position, token, logits and partials are put back after each of the
        two warm-up steps and after the capture.  (The warm-up steps write the cache row of the current position, which the step that
        follows writes anyway.)"""
        saved = [t.clone() for t in self._state()]

        def restore():
            for t, s in zip(self._state(), saved):
                t.copy_(s)
        self._one()
        restore()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._one()
            restore()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._one()
        restore()
        return g

    @torch.no_grad()
    def _prepare(self):
        if not self._want_graph:
            return
        if self._generation is not None:                 # a third launch sequence: its own graph, captured on first use like the sampled one
            if self._generation.pad_id not in self._graphs_generation:
                self._graphs_generation[self._generation.pad_id] = self._capture_in_place()
            return
        if self._sampling is not None:                   # the sampled step is a launch sequence of its own: a second graph, captured on first use
            if self._graph_sampled is None:
                self._graph_sampled = self._capture_in_place()
            return
        if self._graph is not None:
            return
        if self._steps:                                  # first greedy step of an engine that has only sampled so far: nothing may be reset
            self._graph = self._capture_in_place()
            return
        keep = self.ids.clone()
        self._one()                                      # warm-up (allocator, table builds); the caches are rewritten from position 0
        self.reset()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._one()
            self.reset()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._one()
        self.reset()
        self.ids.copy_(keep)
        self._graph = g

    @torch.no_grad()
    def step(self):
        """advance one position from the engine's own state (free-running greedy: the next token is the previous step's argmax)"""
        if self._steps >= self.max_len:
            raise RuntimeError("DecodeEngine: KV cache full (max_len %d)" % self.max_len)
        self._prepare()
        if self._generation is not None:
            g = self._graphs_generation.get(self._generation.pad_id)
        else:
            g = self._graph if self._sampling is None else self._graph_sampled
        if g is not None:
            g.replay()
        else:
            self._one()
        self._steps += 1

    @torch.no_grad()
    def forward(self, ids):
        """feed token ids [bs] (int or tensor) at the next position; returns the logits buffer [bs, vocab] (valid until the next step)"""
        self._prepare()
        if torch.is_tensor(ids):
            self.ids.copy_(ids.reshape(-1))
        else:
            self.ids.fill_(int(ids))
        if self._fh:
            self.part_idx.fill_(-1)                      # teacher-forced: the embed launch reads `ids`, not the previous argmax
        self.step()
        return self.logits

    PREFILL_BYTES = 64 << 20       # default chunk: the widest activation of a pass (bs * chunk rows of the feed-forward width) stays under this

    def _ffn_width(self):
        b = self.dec.blocks[0]
        lin = b.fc1 if hasattr(b, "fc1") else b.gate_proj
        return getattr(lin, "out_features", None) or lin.outfeatures

    def prefill_chunk(self):
        """the default `chunk` of prefill(): the most positions per sequence (a multiple of 64, the attention kernel's query tile) for which
        the feed-forward activation [bs * chunk, ffn] of a pass stays within PREFILL_BYTES; at least 64"""
        item = torch.empty((), dtype=self.dtype).element_size()
        rows = self.PREFILL_BYTES // (self._ffn_width() * item * self.bs)
        return max(64, rows // 64 * 64)

    def _refuse_prompt(self, who, what, prompt_ids, chunk):
        """the refusals of a prompt pass (prefill, score), raised before anything is written; returns (n, chunk)"""
        if not torch.is_tensor(prompt_ids) or prompt_ids.dim() != 2 or prompt_ids.shape[0] != self.bs or prompt_ids.shape[1] < 1:
            shape = tuple(prompt_ids.shape) if torch.is_tensor(prompt_ids) else type(prompt_ids).__name__
            raise ValueError(f"DecodeEngine.{who}: {what} must be int64 [bs = {self.bs}, n >= 1] (got {shape})")
        n = prompt_ids.shape[1]
        if self._steps + n > self.max_len:
            raise RuntimeError(f"DecodeEngine.{who}: a prompt of {n} positions does not fit the KV cache ({self._steps} of max_len "
                               f"{self.max_len} positions are in use)")
        for name, m in self.dec.named_modules():
            if isinstance(m, QuantLinear) and m.qweight.numel() == 0 and m.infeatures * m.outfeatures:
                raise RuntimeError(f"DecodeEngine.{who}: layer {name} went through QuantLinear.decode_only(): it kept the decode-order codes "
                                   "only, and the prompt pass runs the layers' forward on the natural-order codes.  Build the engine from the "
                                   "packed checkpoint without decode_only() (or re-pack the layer), or feed the prompt token by token with forward()")
        if chunk is None:
            chunk = self.prefill_chunk()
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"DecodeEngine.{who}: chunk must be at least 1")
        return n, chunk

    @torch.no_grad()
    def prefill(self, prompt_ids, chunk=None, all_logits=False):
        """feed a whole prompt, int64 [bs, n] with n >= 1, in passes of at most `chunk` positions per sequence (default: prefill_chunk()):
        every block's cache rows pos .. pos + n - 1 are written and the engine advances by n.  The logits of the last prompt position are
        left in `logits` and their argmax in `ids`, so step() / generate() continue from the prompt by graph replay.  On an engine that
        already holds positions the prompt continues the sequence.  Returns `logits` [bs, vocab], or with all_logits the logits of every
        prompt position [bs, n, vocab].  Raises before anything is written when the prompt does not fit the cache, bs is wrong, or a layer
        dropped its natural-order codes (QuantLinear.decode_only)."""
        n, chunk = self._refuse_prompt("prefill", "prompt_ids", prompt_ids, chunk)
        self._prepare()                                  # (its warm-up and capture steps write position 0 and reset: before the first cache write)
        ids = prompt_ids.to(device=self.dev, dtype=torch.int64)
        outs = []
        for lo in range(0, n, chunk):
            part = ids[:, lo:lo + chunk]
            lg = self.dec.prefill(part, self.pos, self.caches, self.arange, all_logits=all_logits)
            self.pos.add_(part.shape[1])                 # the next pass starts behind this one: `start` lives on the device
            if all_logits:
                outs.append(lg)
        last = lg[:, -1] if all_logits else lg
        self.logits.copy_(last)
        if self._generation is not None:                 # the prompt is the history so far; nothing was "just fed" for the launch to record
            self.history[:, self._steps:self._steps + n].copy_(ids)
            self._generate_launch(None)
        elif self._sampling is None:
            ops.argmax_rows(self.logits, out=self.ids)
        else:
            self._sample()                               # pos is behind the prompt by now: the position the drawn token is fed at
        if self._fh:
            self.part_idx.fill_(-1)                      # the next step's embed launch reads `ids`, not the partials of an earlier step
        self._steps += n
        if all_logits:
            return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
        return self.logits

    @torch.no_grad()
    def score(self, ids, targets=None, chunk=None, vocab=None):
        """feed ids int64 [bs, n] from the engine's current position like prefill() -- same passes of `chunk` positions, same defaults, same
        refusals before anything is written, same cache rows, the engine advances by n -- but end every pass in ops.head_score on its
        hidden states instead of the head: no [rows, vocab] tensor is built and no logit is rounded to 16 bits.  Returns (logprob fp32
        [bs, n], greedy int64 [bs, n]): the log-probability of targets[b, t] given ids[b, :t + 1] and the arg-max token of that position.
        targets int64 [bs, n], default the next token (targets[:, t] = ids[:, t + 1], the last position -1); a negative target is an ignored
        position (logprob 0), one at or past the vocabulary gives -inf.  vocab: score against the first `vocab` rows of the head only (the
        reference scores [:, :, :50272] of OPT's padded table).  `logits` and `ids` are left as they were: to generate afterwards, feed a
        token (forward)."""
        n, chunk = self._refuse_prompt("score", "ids", ids, chunk)
        W = self.dec.head_weight
        vocab = W.shape[0] if vocab is None else int(vocab)
        if not 1 <= vocab <= W.shape[0]:
            raise ValueError(f"DecodeEngine.score: vocab {vocab} outside the head's {W.shape[0]} rows")
        if targets is not None and (not torch.is_tensor(targets) or tuple(targets.shape) != (self.bs, n)):
            shape = tuple(targets.shape) if torch.is_tensor(targets) else type(targets).__name__
            raise ValueError(f"DecodeEngine.score: targets must be int64 [bs = {self.bs}, n = {n}] (got {shape})")
        self._prepare()
        ids = ids.to(device=self.dev, dtype=torch.int64)
        if targets is None:
            targets = torch.cat([ids[:, 1:], torch.full((self.bs, 1), -1, dtype=torch.int64, device=self.dev)], dim=1)
        else:
            targets = targets.to(device=self.dev, dtype=torch.int64)
        rows = self.bs * min(chunk, n)
        ws = self.__dict__.get("_score_ws")                  # one workspace per engine: sized for the head's whole table, grown only by a larger pass
        if ws is None or ws[0] < rows:
            ws = (rows, ops.head_score_workspace(rows, W.shape[0], self.dev))
            self.__dict__["_score_ws"] = ws
        logprob = torch.empty((self.bs, n), dtype=torch.float32, device=self.dev)
        greedy = torch.empty((self.bs, n), dtype=torch.int64, device=self.dev)
        for lo in range(0, n, chunk):
            part = ids[:, lo:lo + chunk]
            T = part.shape[1]
            x = self.dec.prefill(part, self.pos, self.caches, self.arange, hidden=True)          # [bs * T, h], row b * T + t
            self.pos.add_(T)
            lp, _, gr = ops.head_score(x, W, targets[:, lo:lo + T].reshape(-1), vocab=vocab, workspace=ws[1])
            logprob[:, lo:lo + T] = lp.view(self.bs, T)
            greedy[:, lo:lo + T] = gr.view(self.bs, T)
        if self._generation is not None:                     # the fed tokens are history, as after prefill(); nothing is drawn here
            self.history[:, self._steps:self._steps + n].copy_(ids)
        if self._fh:
            self.part_idx.fill_(-1)                          # the next step's embed launch reads `ids`, not the partials of an earlier step
        self._steps += n
        return logprob, greedy

    @torch.no_grad()
    def loglikelihood(self, requests, vocab=None):
        """the reference's zero-shot scoring (zeroShot BaseLM._loglikelihood_tokens): requests is a sequence of (context_ids,
        continuation_ids), both non-empty lists of ints; returns [(sum of the continuation's log-probabilities given the context,
        would greedy decoding have produced the continuation)] in request order.  Batching is collate_requests(requests, bs, max_len):
        longest first, bs at a time, inputs cut from the left to max_len, right-padded with token 0 (causal attention keeps the pad out
        of the positions before it), a short last batch filled with copies of its first request.  Every batch is one score() from an empty
        cache and one device-to-host copy; the engine is at position 0 afterwards.  A continuation longer than max_len raises ValueError
        before any GPU work.  vocab: as in score()."""
        batches = collate_requests(requests, self.bs, self.max_len)
        out = [None] * len(requests)
        for b in batches:
            self.reset()
            tg = b.targets.to(self.dev)
            lp, gr = self.score(b.ids.to(self.dev), tg, vocab=vocab)
            hit = ((gr == tg) | (tg < 0)).all(dim=1)
            both = torch.stack([lp.double().sum(dim=1), hit.double()], dim=1).cpu()               # targets < 0 contribute exactly 0
            for r in range(b.real):
                out[b.index[r]] = (float(both[r, 0]), bool(both[r, 1] != 0))
        self.reset()
        return out

    @torch.no_grad()
    def perplexity(self, input_ids, fused=False):
        """the reference's evaluation (opt.py:287-297, llama.py:244-250) on the engine's own layers: input_ids int64 [nsamples, seqlen], every
        sample an independent sequence prefilled from an empty cache (bs samples per pass); shifted cross-entropy in fp32,
        exp(sum nll / (nsamples * seqlen)) with nll = mean CE of the sample * seqlen.  Returns a float.
        fused=True: the mean NLL comes from score() -- fp32 logits inside the head kernel, no [bs, seqlen, vocab] tensor."""
        input_ids = input_ids.to(self.dev)
        if input_ids.dim() != 2 or input_ids.shape[1] < 2:
            raise ValueError("DecodeEngine.perplexity: input_ids must be [nsamples, seqlen >= 2]")
        nsamples, seqlen = input_ids.shape
        if seqlen > self.max_len:
            raise RuntimeError(f"DecodeEngine.perplexity: seqlen {seqlen} > max_len {self.max_len}")
        nlls = []
        for lo in range(0, nsamples, self.bs):
            batch = input_ids[lo:lo + self.bs]
            real = batch.shape[0]
            if real < self.bs:                           # the last pass: pad with copies of its first sample, which are not counted
                batch = torch.cat([batch, batch[:1].expand(self.bs - real, seqlen)])
            self.reset()
            if fused:
                lp, _ = self.score(batch)                # next-token targets; the last position is ignored (0)
                for r in range(real):
                    nlls.append((-lp[r, :-1].double().sum() / (seqlen - 1)).float() * seqlen)
                continue
            lg = self.prefill(batch, all_logits=True)
            for r in range(real):
                loss = F.cross_entropy(lg[r, :-1].float(), batch[r, 1:])
                nlls.append(loss.float() * seqlen)
        self.reset()
        return float(torch.exp(torch.stack(nlls).sum() / (nsamples * seqlen)))

    @torch.no_grad()
    def generate(self, first, n, sampling=None, generation=None):
        """continuation: returns int64 [n, bs] -- the n tokens following `first`.  Greedy (model.generate(do_sample=False) with a cache) unless
        a `Sampling` is in force: the engine's (set_sampling), or `sampling`, which applies to this call only -- the previous setting is put
        back afterwards, also when the call raises.  `generation` does the same for a `Generation` (not both in one call).
        `first`: one token per sequence (int or [bs]), or a prompt [bs, n_prompt], which is prefilled in one pass.
        Under a Generation the result is int64 [n', bs]: a sequence that drew a stop token holds `pad_id` behind it, stepping ends once every
        sequence is finished (the host reads `finished` every `poll` steps -- the one synchronisation this adds), and the result is cut to
        n' = the latest stop's step + 1 whatever `poll` is (n' == n when some sequence never stopped).  `lengths` then holds, per sequence,
        the number of tokens up to and including its stop token (n' if it never stopped)."""
        if sampling is not None and (generation is not None or self._generation is not None):
            raise ValueError("DecodeEngine.generate: sampling= and a Generation exclude each other -- pass generation=Generation(sampling=...)")
        if generation is not None:
            prev = self._generation
            self.set_generation(generation)
            try:
                return self.generate(first, n)
            finally:
                self.set_generation(prev)
        if sampling is not None:
            prev = self._sampling
            self.set_sampling(sampling)
            try:
                return self.generate(first, n)
            finally:
                self.set_sampling(prev)
        if torch.is_tensor(first) and first.dim() == 2 and first.shape[1] > 1:
            self.prefill(first)
        else:
            self.forward(first)
        if self._generation is not None:
            return self._generate_controlled(n)
        out = []
        for i in range(n):
            if self._fh and self._sampling is None:      # the embed launch of step i + 1 writes step i's argmax into `ids`
                if i == n - 1:
                    out.append(self.logits.float().argmax(-1))
                else:
                    self.step()
                    out.append(self.ids.clone())
            else:                                        # the step itself leaves its token (argmax, or the sample launch's draw) in `ids`
                out.append(self.ids.clone())
                if i < n - 1:
                    self.step()
        return torch.stack(out)

    def _generate_controlled(self, n):
        """generate()'s loop under a Generation: token i of the result is the one fed at position c0 + i, so a stop recorded at position
        stop_pos is step stop_pos - c0"""
        c0 = self._steps
        out = []
        for i in range(n):
            out.append(self.ids.clone())
            if i == n - 1:
                break
            if self.poll and (i + 1) % self.poll == 0 and bool(self.finished.all()):
                break
            self.step()
        toks = torch.stack(out) if out else torch.empty((0, self.bs), dtype=torch.int64, device=self.dev)
        done, at = self.finished.cpu(), self.stop_pos.cpu() - c0             # (rows finished before this call: a step below 0)
        stopped = (done != 0) & (at < len(out))
        n_out = int(at[stopped].max().clamp_(min=-1)) + 1 if bool(stopped.all()) and self.bs else len(out)
        self.lengths = torch.where(stopped, (at + 1).clamp_(min=0), torch.full_like(at, n_out))
        return toks[:n_out]

    @torch.no_grad()
    def benchmark(self, input_ids, check=False, verbose=False):
        """opt.py:431-482 / llama.py:418-471: feed `input_ids` [1, n] one token per step, synchronise and time every step; returns
        {'median_s', 'times', 'ppl' (check=True)}"""
        input_ids = input_ids.to(self.dev).reshape(self.bs, -1)
        n = input_ids.shape[1]
        self._prepare()
        self.reset()
        torch.cuda.synchronize()
        times, tot = [], 0.0
        for i in range(n):
            tick = time.time()
            lg = self.forward(input_ids[:, i])
            torch.cuda.synchronize()
            times.append(time.time() - tick)
            if verbose:
                print(i, times[-1])
            if check and i != n - 1:
                tot += F.cross_entropy(lg.float(), input_ids[:, i + 1]).float()
        out = {"median_s": float(np.median(times)), "times": times}
        if check:
            out["ppl"] = float(torch.exp(tot / (n - 1)))
        return out


def benchmark(model, input_ids, check=False, engine=None):
    """drop-in for the reference's `benchmark(model, input_ids, check=False)` (opt.py:431, llama.py:418): same loop, same printout
    ('Median:', 'PPL:'), on the decode engine built over `model` (kept on the model between calls)"""
    eng = engine or getattr(model, "_quip_decode_engine", None)
    n = input_ids.numel()
    if eng is None or eng.max_len < n:
        eng = DecodeEngine.from_hf(model, max_len=max(n, 16))
        model.__dict__["_quip_decode_engine"] = eng
    print('Benchmarking ...')
    res = eng.benchmark(input_ids, check=check, verbose=True)
    print('Median:', res["median_s"])
    if check:
        print('PPL:', res["ppl"])
    return res


def perplexity(model, testenc, engine=None, fused=False):
    """the reference's `opt_eval` / `llama_eval` figure (opt.py:194-297, llama.py:175-251) on the decode engine built over `model` (kept on
    the model between calls): testenc is the tokenised test set ([1, N] ids, or the tokenizer's output with .input_ids), cut into
    N // model.seqlen samples of model.seqlen tokens; prints and returns the perplexity.  fused: DecodeEngine.perplexity's flag"""
    ids = getattr(testenc, "input_ids", testenc)
    seqlen = int(model.seqlen)
    nsamples = ids.numel() // seqlen
    ids = ids.reshape(-1)[:nsamples * seqlen].reshape(nsamples, seqlen)
    eng = engine or getattr(model, "_quip_decode_engine", None)
    if eng is None or eng.max_len < seqlen:
        eng = DecodeEngine.from_hf(model, max_len=seqlen)
        model.__dict__["_quip_decode_engine"] = eng
    print('Evaluating ...')
    ppl = eng.perplexity(ids, fused=True) if fused else eng.perplexity(ids)
    print(ppl)
    return ppl


ScoreBatch = collections.namedtuple("ScoreBatch", "ids targets index real")


def collate_requests(requests, bs, max_len):
    """the batching of the reference's zero-shot scoring, as a pure function (no GPU): requests is a sequence of (context_ids,
    continuation_ids), both non-empty lists of ints.  The requests are ordered by (-len(ctx + cont), tuple(ctx + cont)) and taken bs at a
    time; a request's input is (ctx + cont)[-(max_len + 1):][:-1], right-padded with token 0 to the batch's first (longest) input; its
    targets are the continuation on the last len(cont) input positions and -1 everywhere else (the pad included).  A short last batch is
    filled with copies of its first request.  Returns [ScoreBatch(ids int64 [bs, n], targets int64 [bs, n], index: the request index of
    every row, real: how many leading rows are requests of their own)].  ValueError for an empty context or continuation and for a
    continuation longer than max_len."""
    reqs = []
    for i, (ctx, cont) in enumerate(requests):
        ctx, cont = [int(t) for t in ctx], [int(t) for t in cont]
        if not ctx or not cont:
            raise ValueError(f"collate_requests: request {i} has an empty context or continuation")
        if len(cont) > max_len:
            raise ValueError(f"collate_requests: the continuation of request {i} has {len(cont)} tokens, more than max_len {max_len}")
        reqs.append((i, ctx + cont, cont))
    reqs.sort(key=lambda r: (-len(r[1]), tuple(r[1])))
    batches = []
    for lo in range(0, len(reqs), bs):
        group = reqs[lo:lo + bs]
        real = len(group)
        group = group + [group[0]] * (bs - real)
        inputs = [toks[-(max_len + 1):][:-1] for _, toks, _ in group]
        n = len(inputs[0])
        ids = torch.zeros((bs, n), dtype=torch.int64)
        targets = torch.full((bs, n), -1, dtype=torch.int64)
        for r, (inp, (_, _, cont)) in enumerate(zip(inputs, group)):
            ids[r, :len(inp)] = torch.tensor(inp, dtype=torch.int64)
            targets[r, len(inp) - len(cont):len(inp)] = torch.tensor(cont, dtype=torch.int64)
        batches.append(ScoreBatch(ids, targets, [g[0] for g in group], real))
    return batches


def loglikelihood(model, requests, engine=None, bs=1):
    """the reference's zero-shot scoring (zeroShot BaseLM._loglikelihood_tokens) on the decode engine built over `model` (kept on the
    model between calls, like perplexity): requests is a sequence of (context_ids, continuation_ids) token lists -- no tokenizer is
    needed --; returns [(log-likelihood of the continuation, is it the greedy continuation)] in request order.  The context window is
    model.seqlen when set, else the model's max_position_embeddings."""
    eng = engine or getattr(model, "_quip_decode_engine", None)
    if eng is None or (engine is None and eng.bs != bs):
        max_len = int(getattr(model, "seqlen", 0) or model.config.max_position_embeddings)
        eng = DecodeEngine.from_hf(model, bs=bs, max_len=max_len)
        model.__dict__["_quip_decode_engine"] = eng
    return eng.loglikelihood(requests)
