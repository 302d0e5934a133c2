"""-m gpu: the decode attention launches at the context lengths the models have, against an fp64 reference built independently of the
repo's kernels.

  1. quipamd_decode_attention_fused (csrc/decode_attn.hip: mode v3's attention for every packed OPT and Llama block) -- its three
     instantiations x its three forms (one head per 12-wave workgroup, three heads per workgroup, the 4-wave form, forced through
     ops.decode_attention_config) at maxlen 64, 4096 and each form's LDS limit and one past it, at positions 0, 255, 256 (the edge of the
     prefetched first K rows), a middle one and maxlen - 1; random caches and "needle" caches whose one K row is a large multiple of the
     query, so that softmax sits on that row and a launch that reads the wrong rows fails outright instead of averaging away;
  2. the form the launch picks by itself at 9 x 32 and 17 x 16 (sequence, head) pairs, just inside and past the three-heads form's limit;
  3. quipamd_decode_attention (plain) and quipamd_decode_attention_grouped at their 32768-position cap.

Reference (1, 2): q, k, v = U^T y + bias in fp64 from the operators' generator tuples (test_gpu_decode_fused._dense) on natural-order y,
HF's rotate_half in fp64 at pos, this token's k / v appended, softmax attention over positions 0..pos in fp64.  Gates: output within 3e-3
and the appended k / v rows within 2e-3 (relative l2, the worst (sequence, head)); every other cache row and head bit for bit unchanged;
the forms bit for bit equal; past the one-head form's limit the launch is refused (QUIPAMD_ERR_SHAPE) and the caches are left as they
were.  Limits come from ops.decode_attention_fused_max_len and the LDS rule of test_decode_attn_host.py."""
import math
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_decode_attn_host import form_max_len                        # noqa: E402  (the LDS rule, restated)
from test_gpu_decode_fused import _dense, _layer                       # noqa: E402

NEEDLE = 16.0             # a needle row's score: e^16 outweighs the ~e^0 of every other row of a 26384-position cache by ~300x
INSTS = {                 # n = heads x hd (the operator is 64 x 32 at n 2048, 64 x 64 at 4096), heads, hd, rotary
    "hd64-64x32": (2048, 32, 64, False),
    "hd128-64x64": (4096, 32, 128, True),
    "hd128-64x32": (2048, 16, 128, True),           # 16 heads: the last three-heads workgroup holds one live head and two idle ones
}
FORMS = {"one_head": (0, 0), "three_heads": (0, 1), "four_wave": (1, 0)}    # ops.decode_attention_config(one_group_from, three_heads_from)

_ops = {}


def _inst(name):
    """the three packed q / k / v layers of an instantiation and their transposed output-side operators as dense fp64 matrices"""
    n, heads, hd, rope = INSTS[name]
    if n not in _ops:
        qkv = [_layer(n, n, 700 + i + n % 13)[0] for i in range(3)]
        _ops[n] = (qkv, [_dense(l.U, transpose=True) for l in qkv])
    qkv, Ut = _ops[n]
    return types.SimpleNamespace(qkv=qkv, Ut=Ut, n=n, heads=heads, hd=hd, rope=rope, p=qkv[0].U.p, q=qkv[0].U.q)


def _rotary64(hd, rows):
    """HF's cos / sin (duplicated halves) in fp64; the launch gets them rounded to fp32"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    fr = torch.outer(torch.arange(rows, dtype=torch.float64), inv)
    emb = torch.cat((fr, fr), -1).to(DEV)
    return emb.cos(), emb.sin()


def _qkv64(I, ys, pos, tab64):
    """this step's q, k, v [bs, heads, hd] in fp64: U^T y + bias, rotate_half rotary on q and k"""
    bs = ys[0].shape[0]
    q, k, v = ((y.double() @ Ut.t() + l.bias.half().double()).view(bs, I.heads, I.hd) for l, Ut, y in zip(I.qkv, I.Ut, ys))
    if I.rope:
        c, s = tab64[0][pos], tab64[1][pos]
        h = I.hd // 2
        rot = lambda x: x * c + torch.cat((-x[..., h:], x[..., :h]), -1) * s
        q, k = rot(q), rot(k)
    return q, k, v


def _attn64(q, k, v, kc, vc, pos):
    K, V = kc[:, :, :pos + 1].double(), vc[:, :, :pos + 1].double()
    K[:, :, pos], V[:, :, pos] = k, v
    s = torch.einsum("bhd,bhtd->bht", q, K) / math.sqrt(q.shape[-1])
    return torch.einsum("bht,bhtd->bhd", torch.softmax(s, -1), V)


def _needle(kc, q, npos):
    """a copy of kc whose row npos is the multiple of q that scores NEEDLE, for every (sequence, head)"""
    kc = kc.clone()
    a = NEEDLE * math.sqrt(q.shape[-1]) / (q * q).sum(-1, keepdim=True)
    kc[:, :, npos] = (a * q).to(kc.dtype)
    return kc


def _rel(got, want):
    """relative l2 error of the worst (sequence, head): [.., heads, hd] tensors"""
    got = got.double().reshape(want.shape)
    return float(((got - want).norm(dim=-1) / want.norm(dim=-1)).max())


def _fused(I, ys, kc, vc, pos, tabs, form=None):
    """one fused launch on copies of the caches; form: a FORMS key, None = the launch's own choice.  Returns (out, kc, vc)."""
    from quip_amd import ops
    from quip_amd.quant import fused_attention
    kc, vc = kc.clone(), vc.clone()
    try:
        if form is not None:
            ops.decode_attention_config(*FORMS[form])
        out = fused_attention(I.qkv, [l.to_zt(y) for l, y in zip(I.qkv, ys)], kc, vc, torch.tensor([pos], device=DEV), *tabs)
        torch.cuda.synchronize()
    finally:
        ops.decode_attention_config()
    return out, kc, vc


def _check(I, ys, kc0, vc0, pos, tabs, tab64, forms, report, npos=None):
    """forms run on the same inputs: the first against fp64, the others bit for bit equal to it"""
    q, k, v = _qkv64(I, ys, pos, tab64)
    kc_in = kc0 if npos is None else _needle(kc0, q, npos)
    want = _attn64(q, k, v, kc_in, vc0, pos)
    runs = [_fused(I, ys, kc_in, vc0, pos, tabs, f) for f in forms]
    out, kc, vc = runs[0]
    e_out, e_kv = _rel(out, want), max(_rel(kc[:, :, pos], k), _rel(vc[:, :, pos], v))
    key = "needle" if npos is not None else "random"
    report[key] = (max(report.get(key, (0, 0))[0], e_out), max(report.get(key, (0, 0))[1], e_kv))
    assert e_out <= 3e-3, (pos, npos, e_out)
    assert e_kv <= 2e-3, (pos, npos, e_kv)
    for c, c0 in ((kc, kc_in), (vc, vc0)):                             # nothing but row pos of every (sequence, head) written
        c = c.clone()
        c[:, :, pos] = c0[:, :, pos]
        assert torch.equal(c, c0), (pos, npos)
    for f, other in zip(forms[1:], runs[1:]):
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other)), (f, pos, npos)
    return runs[0]


def _inputs(I, bs, maxlen, seed):
    torch.manual_seed(seed)
    kc0 = (0.5 * torch.randn(bs, I.heads, maxlen, I.hd, device=DEV)).half()
    vc0 = (0.5 * torch.randn(bs, I.heads, maxlen, I.hd, device=DEV)).half()
    ys = [(0.5 * torch.randn(bs, I.n, device=DEV)).half() for _ in range(3)]
    tab64 = _rotary64(I.hd, maxlen) if I.rope else None
    tabs = (tab64[0].float().contiguous(), tab64[1].float().contiguous()) if I.rope else (None, None)
    return kc0, vc0, ys, tab64, tabs


def _limits(I):
    """(maxlen, what) cases of an instantiation: 64, 4096, each form's LDS limit and one past it"""
    from quip_amd import ops
    one = ops.decode_attention_fused_max_len(I.hd, I.p, I.q)
    three = form_max_len(I.hd, I.p, I.q, True)
    assert one == form_max_len(I.hd, I.p, I.q, False) and 0 < three < one
    return {"64": 64, "4096": 4096, "mh": three, "mh+1": three + 1, "one": one, "one+1": one + 1}


@pytest.mark.parametrize("which", ["64", "4096", "mh", "mh+1", "one"])
@pytest.mark.parametrize("name", list(INSTS))
def test_fused_attention_matches_fp64_at_every_context_length(name, which):
    I = _inst(name)
    maxlen = _limits(I)[which]
    bs = 2
    kc0, vc0, ys, tab64, tabs = _inputs(I, bs, maxlen, maxlen + I.n)
    report = {}
    for pos in sorted({0, 255, 256, maxlen // 2 + 1, maxlen - 1} & set(range(maxlen))):
        for npos in [None] + sorted({0, 255, 256, pos - 1} & set(range(pos))):
            _check(I, ys, kc0, vc0, pos, tabs, tab64, list(FORMS), report, npos)
    print(f"fused attention {name} maxlen {maxlen} ({which}): worst (out rel err, appended k/v rel err) vs fp64 {report}, gates (3e-3, 2e-3)")


@pytest.mark.parametrize("name", list(INSTS))
def test_fused_attention_refuses_a_cache_past_every_form(name):
    from quip_amd import _lib, ops
    from quip_amd.quant import fused_attention
    I = _inst(name)
    maxlen = _limits(I)["one+1"]
    kc0, vc0, ys, _, tabs = _inputs(I, 1, maxlen, 5)
    kc, vc = kc0.clone(), vc0.clone()
    for form in FORMS:
        try:
            ops.decode_attention_config(*FORMS[form])
            with pytest.raises(_lib.QuipAmdError, match="LDS") as e:
                fused_attention(I.qkv, [l.to_zt(y) for l, y in zip(I.qkv, ys)], kc, vc, torch.tensor([maxlen - 1], device=DEV), *tabs)
        finally:
            ops.decode_attention_config()
        torch.cuda.synchronize()
        assert "code 2" in str(e.value), str(e.value)
        assert torch.equal(kc, kc0) and torch.equal(vc, vc0)


@pytest.mark.parametrize("name,bs,which", [("hd128-64x64", 9, "mh"), ("hd128-64x64", 9, "mh+1"), ("hd128-64x64", 9, 4096),
                                           ("hd128-64x32", 17, "mh"), ("hd128-64x32", 17, "mh+1")])
def test_default_form_serves_every_pair_count(name, bs, which):
    """more than 256 (sequence, head) pairs: the launch's own choice is the three-heads form where its LDS fits and the one-head form past
    that -- it used to take the three-heads form regardless and refuse the cache (Llama-2-7B from 9 sequences at its 4096 context)"""
    I = _inst(name)
    three = form_max_len(I.hd, I.p, I.q, True)
    maxlen = which if isinstance(which, int) else three + (which == "mh+1")
    assert bs * I.heads >= 257
    kc0, vc0, ys, tab64, tabs = _inputs(I, bs, maxlen, maxlen + bs)
    expect = "three_heads" if maxlen <= three else "one_head"
    report = {}
    for pos, npos in ((256, None), (maxlen - 1, None), (maxlen - 1, maxlen - 2), (maxlen - 1, 255)):
        default = _check(I, ys, kc0, vc0, pos, tabs, tab64, [None], report, npos)
        forced = _fused(I, ys, kc0 if npos is None else _needle(kc0, _qkv64(I, ys, pos, tab64)[0], npos), vc0, pos, tabs, expect)
        assert all(torch.equal(a, b) for a, b in zip(default, forced)), (pos, npos)
    print(f"fused attention {name}, {bs} sequences, maxlen {maxlen}, own choice (= {expect}): worst errors vs fp64 {report}")


# ---------------------------------------------------------------------------------------------------------- 3. the other two kernels
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_plain_attention_at_its_cap(dtype, hd):
    """quipamd_decode_attention at 32768 positions, the last one, the first of the last 256-row pass and the one before it"""
    from quip_amd import ops
    from test_gpu_decode_attn import _ref
    bs, heads, maxlen = 1, 4, 32768
    g = torch.Generator().manual_seed(hd)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(DEV)
    q, k, v = mk(bs, heads * hd), mk(bs, heads * hd), mk(bs, heads * hd)
    kc0, vc0 = mk(bs, heads, maxlen, hd), mk(bs, heads, maxlen, hd)
    tol = 2e-3 if dtype == torch.float16 else 1.6e-2                       # test_gpu_decode_attn.py's gate (the output rounding) ...
    rtol = 2e-3 if dtype == torch.float16 else 8e-3                        # ... and relative l2: the output is ~1/sqrt(T) of the rows here
    worst = 0.0
    for pos in (32767, 32512, 32511):
        for npos in (None, 0, 255, 256, pos - 1):
            kc_in = kc0 if npos is None else _needle(kc0, q.double().view(bs, heads, hd), npos)
            want, kc_w, vc_w = _ref(q, k, v, kc_in, vc0, pos)
            kc, vc = kc_in.clone(), vc0.clone()
            got = ops.decode_attention(q, k, v, kc, vc, torch.tensor([pos], dtype=torch.int64, device=DEV))
            assert torch.equal(kc, kc_w) and torch.equal(vc, vc_w)
            assert (got.double() - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())
            rel = _rel(got.view(bs, heads, hd), want.view(bs, heads, hd))
            worst = max(worst, rel)
            assert rel <= rtol, (pos, npos, rel)
    print(f"plain attention hd {hd} {dtype} at maxlen 32768: worst rel err {worst:.2e} (gate {rtol})")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("maxlen,pos", [(32768, 32767), (4097, 4096)])
def test_grouped_attention_at_its_cap(maxlen, pos, g, dtype):
    """quipamd_decode_attention_grouped merging 128 chunk partials (32768 positions), and a last chunk of one position (4097); run-to-run
    bit identity on a reused workspace"""
    from quip_amd import ops
    from test_gpu_decode_gqa import _ref
    bs, kv, hd = 2, 2, 128
    heads = kv * g
    gen = torch.Generator().manual_seed(maxlen + g)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)
    q, k, v = mk(bs, heads * hd), mk(bs, kv * hd), mk(bs, kv * hd)
    kc0, vc0 = mk(bs, kv, maxlen, hd), mk(bs, kv, maxlen, hd)
    tol = 2e-3 if dtype == torch.float16 else 1.6e-2
    rtol = 2e-3 if dtype == torch.float16 else 8e-3
    p = torch.tensor([pos], dtype=torch.int64, device=DEV)
    ws = ops.decode_attention_grouped_workspace(bs, heads, kv, hd, maxlen, DEV)
    worst = 0.0
    for npos in (None, 0, pos - 1):
        kc_in = kc0
        if npos is not None:                                               # the needle for the group's first query head
            kc_in = _needle(kc0, q.double().view(bs, kv, g, hd)[:, :, 0], npos)
        want, kc_w, vc_w = _ref(q, k, v, kc_in, vc0, pos, g)
        kc, vc = kc_in.clone(), vc0.clone()
        got = ops.decode_attention_grouped(q, k, v, kc, vc, p)
        assert torch.equal(kc, kc_w) and torch.equal(vc, vc_w)
        assert (got.double() - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())
        rel = _rel(got.view(bs, heads, hd), want.view(bs, heads, hd))
        worst = max(worst, rel)
        assert rel <= rtol, (npos, rel)
        kc2, vc2 = kc_in.clone(), vc0.clone()
        r1 = ops.decode_attention_grouped(q, k, v, kc2, vc2, p, workspace=ws)
        r2 = ops.decode_attention_grouped(q, k, v, kc2, vc2, p, workspace=ws)
        assert torch.equal(r1, got) and torch.equal(r2, got)
    print(f"grouped attention g {g} {dtype} maxlen {maxlen} pos {pos}: worst rel err {worst:.2e} (gate {rtol})")
