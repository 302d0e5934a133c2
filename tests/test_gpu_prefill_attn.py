"""-m gpu: the prompt-side attention op alone (ops.prefill_attention -> quipamd_prefill_attention, csrc/prefill_attn.hip).

  1. against fp64 causal attention over HF's repeat_kv, under the attention gate of test_gpu_decode_attn.py / test_gpu_decode_gqa.py
     (2e-3 f16 / 1.6e-2 bf16 of max(1, |want|max): the same output rounding, the same gate), with the cache append checked exactly;
  2. the append bit for bit against ops.rope_inplace per position + a plain copy; q, k, v and every other cache row bit-unchanged;
  3. chunking invariance, bit for bit: the result of a row depends on its absolute position only;
  4. strided q / k / v, out-of-range starts, run-to-run identity, hipGraph replay with the start moved on the device."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import prefill_ref as R  # noqa: E402

MAXLEN = 512
SPANS = [(0, 1), (0, 17), (0, 63), (0, 64), (0, 65), (0, 300), (37, 100), (511, 1), (MAXLEN - 70, 70)]      # (start, T); the last ends at maxlen


def _inputs(dtype, hd, g, bs, maxlen, T, seed, kv=None):
    kv = kv or (2 if g > 4 else 3)
    heads = kv * g
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)
    return mk(bs * T, heads * hd), mk(bs * T, kv * hd), mk(bs * T, kv * hd), mk(bs, kv, maxlen, hd), mk(bs, kv, maxlen, hd), kv, heads


def _start(s):
    return torch.tensor([s], dtype=torch.int64, device=DEV)


def _check(dtype, hd, g, bs, maxlen, start, T, rot, seed, kv=None):
    from quip_amd import ops
    q, k, v, kc, vc, kv, heads = _inputs(dtype, hd, g, bs, maxlen, T, seed, kv)
    cos = sin = None
    if rot:
        cos, sin = (t.to(DEV) for t in R.tables(hd, maxlen))
    q0, k0, v0 = q.clone(), k.clone(), v.clone()
    kc_w, vc_w = R.append_want(k, v, kc, vc, start, T, cos, sin)
    qr = R.rope(q, cos, sin, start, T, heads) if rot else q
    want = R.causal_fp64(qr, kc_w, vc_w, start, T, g)
    got = ops.prefill_attention(q, k, v, kc, vc, _start(start), T, cos, sin)
    assert got.shape == (bs * T, heads * hd) and got.dtype == dtype and got.is_contiguous()
    assert torch.equal(kc, kc_w) and torch.equal(vc, vc_w), "cache append: rows [start, start + T) exact, every other row unchanged"
    assert torch.equal(q, q0) and torch.equal(k, k0) and torch.equal(v, v0), "q / k / v are inputs"
    ok, frac = R.within_gate(got, want, dtype)
    print(f"{dtype} hd {hd} g {g} bs {bs} maxlen {maxlen} start {start} T {T} rot {rot}: {frac:.3f} of the gate")
    assert ok, f"{frac:.3f} of the gate at start {start} T {T}"
    again = ops.prefill_attention(q, k, v, kc, vc, _start(start), T, cos, sin)          # the same bits again, caches included
    assert torch.equal(again, got) and torch.equal(kc, kc_w) and torch.equal(vc, vc_w)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("g", [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize("bs", [1, 3])
def test_matches_fp64_causal_attention_over_repeat_kv(dtype, hd, g, bs):
    for i, (start, T) in enumerate(SPANS):
        rot = (i + bs + g) % 2 == 0                                          # with and without rotary tables across the grid
        _check(dtype, hd, g, bs, MAXLEN, start, T, rot, seed=1000 * i + 7 * g + hd + bs)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("start,T", [(0, 2048), (2048, 2048), (4000, 96)])
def test_long_prompts_at_4096(dtype, start, T):
    _check(dtype, 128, 8, 2, 4096, start, T, True, seed=start + T)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_the_end_of_a_32768_context(dtype):
    _check(dtype, 128, 2, 1, 32768, 32000, 768, True, seed=5, kv=1)


@pytest.mark.parametrize("dtype,hd,g,start,T", [(torch.float16, 128, 1, 0, 70), (torch.bfloat16, 64, 4, 37, 100), (torch.float16, 64, 2, 200, 33)])
def test_append_is_rope_inplace_per_position_then_a_copy(dtype, hd, g, start, T):
    """the written K rows are bit-identical to ops.rope_inplace called once per position on that position's rows, V rows to v itself"""
    from quip_amd import ops
    bs = 2
    q, k, v, kc, vc, kv, heads = _inputs(dtype, hd, g, bs, MAXLEN, T, seed=start + T)
    cos, sin = (t.to(DEV) for t in R.tables(hd, MAXLEN))
    qr, kr = q.clone(), k.clone()
    for t in range(T):                                                       # rows b T + t of every sequence sit at position start + t
        ops.rope_inplace(qr.view(bs, T, -1)[:, t], kr.view(bs, T, -1)[:, t], cos, sin, _start(start + t), heads, kv)
    kc_w, vc_w = kc.clone(), vc.clone()
    kc_w[:, :, start:start + T] = kr.view(bs, T, kv, hd).transpose(1, 2)
    vc_w[:, :, start:start + T] = v.view(bs, T, kv, hd).transpose(1, 2)
    assert torch.equal(R.rope(k, cos, sin, start, T, kv), kr)              # (and the torch restatement the other tests use is the same bits)
    got = ops.prefill_attention(q, k, v, kc, vc, _start(start), T, cos, sin)
    assert torch.equal(kc, kc_w) and torch.equal(vc, vc_w)
    want = R.causal_fp64(qr, kc_w, vc_w, start, T, g)
    assert R.within_gate(got, want, dtype)[0]
    # without tables the rows are k and v themselves
    kc2, vc2 = kc_w.clone(), vc_w.clone()
    ops.prefill_attention(q, k, v, kc2, vc2, _start(start), T)
    assert torch.equal(kc2[:, :, start:start + T], k.view(bs, T, kv, hd).transpose(1, 2)) and torch.equal(vc2, vc_w)
    kc2[:, :, start:start + T] = kc_w[:, :, start:start + T]
    assert torch.equal(kc2, kc_w)


@pytest.mark.parametrize("dtype,hd,g,rot,start", [(torch.float16, 128, 1, False, 0), (torch.bfloat16, 128, 4, True, 0), (torch.float16, 64, 3, True, 0),
                                                  (torch.float16, 128, 8, True, 101)])
def test_chunking_is_bit_invariant(dtype, hd, g, rot, start):
    """one call with T = 300 against 128 + 128 + 44 and against 1 + 299: out and caches bit for bit (K tiles sit at absolute positions)"""
    from quip_amd import ops
    bs, T = 2, 300
    q, k, v, kc, vc, kv, heads = _inputs(dtype, hd, g, bs, MAXLEN, T, seed=hd + g)
    cos = sin = None
    if rot:
        cos, sin = (t.to(DEV) for t in R.tables(hd, MAXLEN))
    kc1, vc1 = kc.clone(), vc.clone()
    whole = ops.prefill_attention(q, k, v, kc1, vc1, _start(start), T, cos, sin)
    rows = lambda x, lo, n: x.view(bs, T, -1)[:, lo:lo + n].reshape(bs * n, -1)
    for cuts in ((128, 128, 44), (1, 299), (64, 64, 64, 64, 44), (7, 293)):
        kc2, vc2 = kc.clone(), vc.clone()
        pos = _start(start)
        parts, lo = [], 0
        for n in cuts:
            o = ops.prefill_attention(rows(q, lo, n), rows(k, lo, n), rows(v, lo, n), kc2, vc2, pos, n, cos, sin)
            parts.append(o.view(bs, n, -1))
            pos.add_(n)                                                      # the next chunk starts behind this one, on the device
            lo += n
        got = torch.cat(parts, dim=1).reshape(bs * T, -1)
        assert torch.equal(got, whole), f"out differs for cuts {cuts}"
        assert torch.equal(kc2, kc1) and torch.equal(vc2, vc1), f"caches differ for cuts {cuts}"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_strided_q_k_v_as_column_windows_of_one_tensor(dtype):
    from quip_amd import ops
    bs, T, hd, kv, g, start = 3, 45, 128, 2, 4, 19
    heads = kv * g
    gen = torch.Generator().manual_seed(3)
    qkv = torch.randn(bs * T, (heads + 2 * kv) * hd, generator=gen).to(dtype).to(DEV)
    q, k, v = qkv[:, :heads * hd], qkv[:, heads * hd:(heads + kv) * hd], qkv[:, (heads + kv) * hd:]
    assert not q.is_contiguous() and q.stride(0) == (heads + 2 * kv) * hd
    kc = torch.randn(bs, kv, MAXLEN, hd, generator=gen).to(dtype).to(DEV)
    vc = torch.randn(bs, kv, MAXLEN, hd, generator=gen).to(dtype).to(DEV)
    cos, sin = (t.to(DEV) for t in R.tables(hd, MAXLEN))
    kc2, vc2, keep = kc.clone(), vc.clone(), qkv.clone()
    got = ops.prefill_attention(q, k, v, kc, vc, _start(start), T, cos, sin)
    dense = ops.prefill_attention(q.contiguous(), k.contiguous(), v.contiguous(), kc2, vc2, _start(start), T, cos, sin)
    assert torch.equal(got, dense) and torch.equal(kc, kc2) and torch.equal(vc, vc2) and torch.equal(qkv, keep)
    want = R.causal_fp64(R.rope(q.contiguous(), cos, sin, start, T, heads), kc, vc, start, T, g)
    assert R.within_gate(got, want, dtype)[0]


def test_out_of_range_start_leaves_everything_untouched():
    from quip_amd import ops
    bs, kv, g, hd, maxlen, T = 2, 2, 4, 64, 300, 20
    for start in (-1, -20, 281, 300, 5000):                                  # start < 0 or start + T > maxlen
        kc = torch.ones(bs, kv, maxlen, hd, dtype=torch.float16, device=DEV)
        vc = kc.clone()
        q = torch.ones(bs * T, kv * g * hd, dtype=torch.float16, device=DEV)
        x = torch.full((bs * T, kv * hd), 2.0, dtype=torch.float16, device=DEV)
        ops.prefill_attention(q, x, x, kc, vc, _start(start), T)
        torch.cuda.synchronize()
        assert bool((kc == 1).all()) and bool((vc == 1).all()) and bool((q == 1).all()) and bool((x == 2).all())
    kc = torch.ones(bs, kv, maxlen, hd, dtype=torch.float16, device=DEV)      # start + T == maxlen is in range
    vc = kc.clone()
    ops.prefill_attention(q, x, x, kc, vc, _start(280), T)
    assert bool((kc[:, :, 280:] == 2).all()) and bool((kc[:, :, :280] == 1).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_graph_replay_follows_the_start_on_the_device(dtype):
    """the launches are captured once; between replays only device memory changes (the inputs and *start)"""
    from quip_amd import ops
    bs, kv, g, hd, maxlen, T = 2, 2, 4, 128, 512, 50
    heads = kv * g
    cos, sin = (t.to(DEV) for t in R.tables(hd, maxlen))
    gen = torch.Generator().manual_seed(11)
    mk = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)
    chunks = [(mk(bs * T, heads * hd), mk(bs * T, kv * hd), mk(bs * T, kv * hd)) for _ in range(4)]
    kc, vc = torch.zeros(bs, kv, maxlen, hd, dtype=dtype, device=DEV), torch.zeros(bs, kv, maxlen, hd, dtype=dtype, device=DEV)
    q, k, v = (t.clone() for t in chunks[0])
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.zeros(bs * T, heads * hd, dtype=dtype, device=DEV)

    def step():
        out.copy_(ops.prefill_attention(q, k, v, kc, vc, pos, T, cos, sin))
        pos.add_(T)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    kc.zero_(), vc.zero_()
    for first in (0, 133):                                                   # an aligned walk, then one that starts mid-tile
        pos.fill_(first)
        kr, vr = kc.clone(), vc.clone()
        for i, (cq, ck, cv) in enumerate(chunks):
            q.copy_(cq), k.copy_(ck), v.copy_(cv)
            graph.replay()
            want = ops.prefill_attention(cq, ck, cv, kr, vr, _start(first + i * T), T, cos, sin)
            assert torch.equal(out, want) and torch.equal(kc, kr) and torch.equal(vc, vr)
        assert int(pos) == first + 4 * T
        ok, _ = R.within_gate(out, R.causal_fp64(R.rope(chunks[-1][0], cos, sin, first + 3 * T, T, heads), kc, vc, first + 3 * T, T, g), dtype)
        assert ok
