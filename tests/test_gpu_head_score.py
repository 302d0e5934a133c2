"""-m gpu: ops.head_score (quip_amd/csrc/head_score.hip) against fp64 on the CPU.

Inputs: x ~ N(0, 1), W ~ N(0, 1 / h) from a CPU torch.Generator, rounded to the dtype; the reference is fp64 on the CPU from the same
rounded inputs.  The tolerance is measured, not fixed: the max-abs error of logprob and of lse against fp64 must not exceed the max-abs
error of the torch chain the op replaces (F.linear in the dtype, then .float() log_softmax and gather) on the same inputs -- the kernel
keeps the logits in fp32 where the chain rounds them to 16 bits.
greedy is compared on every row whose fp64 top-2 gap exceeds tau_r = 2 h 2^-24 max_j sum_i |x_ri W_ji| (twice the fp32 summation bound);
at most 2 % of the rows may fall under it.
The bit-for-bit cases (a vocabulary shorter than the table, rows split over calls, a strided x, a repeated call) need no reference."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16

# rows, h, vocab; the seed of a shape is its index here
SHAPES = [(200, 256, 1000), (64, 64, 257), (130, 512, 32000), (96, 128, 50272), (1, 256, 1000), (17, 256, 1000)]


@functools.lru_cache(maxsize=None)
def _case(rows, h, vocab, dtype, seed):
    """(x, W, targets) on the CPU in the dtype, and the fp64 reference (logprob, lse, argmax, decisive rows): computed once per case"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, h, generator=g).to(dtype)
    W = (torch.randn(vocab, h, generator=g) / h ** 0.5).to(dtype)
    t = torch.randint(0, vocab, (rows,), generator=g)
    z = x.double() @ W.double().T
    lse = torch.logsumexp(z, dim=1)
    lp = z.gather(1, t[:, None])[:, 0] - lse
    top2 = z.topk(min(2, vocab), dim=1).values
    gap = top2[:, 0] - top2[:, -1] if vocab > 1 else torch.full((rows,), float("inf"), dtype=torch.float64)
    tau = 2 * h * 2.0 ** -24 * (x.double().abs() @ W.double().abs().T).max(dim=1).values
    return x, W, t, lp, lse, z.argmax(dim=1), gap > tau


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("seed,shape", list(enumerate(SHAPES)))
def test_head_score_is_no_worse_than_the_chain_it_replaces(dtype, seed, shape):
    from quip_amd import ops
    rows, h, vocab = shape
    x, W, t, lp_w, lse_w, arg_w, decisive = _case(rows, h, vocab, dtype, seed)
    xd, Wd, td = x.to(DEV), W.to(DEV), t.to(DEV)
    lp, lse, greedy = ops.head_score(xd, Wd, td)
    chain = F.linear(xd, Wd).float()
    c_lse = torch.logsumexp(chain, dim=1)
    c_lp = torch.log_softmax(chain, dim=1).gather(1, td[:, None])[:, 0]
    err = lambda got, want: (got.double().cpu() - want).abs().max().item()
    e_lp, e_lse, b_lp, b_lse = err(lp, lp_w), err(lse, lse_w), err(c_lp, lp_w), err(c_lse, lse_w)
    left_out = int((~decisive).sum())
    print(f"{dtype} {shape}: logprob err {e_lp:.3e} (chain {b_lp:.3e}), lse err {e_lse:.3e} (chain {b_lse:.3e}), "
          f"{left_out} of {rows} rows under the greedy gap")
    assert lp.dtype == lse.dtype == torch.float32 and greedy.dtype == torch.int64
    assert e_lp <= b_lp, (e_lp, b_lp)
    assert e_lse <= b_lse, (e_lse, b_lse)
    assert left_out <= 0.02 * rows, left_out
    assert torch.equal(greedy.cpu()[decisive], arg_w[decisive])
    assert bool(((greedy >= 0) & (greedy < vocab)).all())


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_ignored_and_out_of_range_targets(dtype):
    from quip_amd import ops
    rows, h, vocab = SHAPES[0]
    x, W, t, lp_w, lse_w, arg_w, decisive = _case(rows, h, vocab, dtype, 0)
    xd, Wd = x.to(DEV), W.to(DEV)
    base = ops.head_score(xd, Wd, t.to(DEV))
    t2 = t.clone()
    t2[0::3] = -1
    t2[1::3] = vocab + torch.arange(t2[1::3].numel()) * 1000          # vocab, vocab + 1000, ...
    t2[4] = -(2 ** 40)
    t2[7] = 2 ** 40
    lp, lse, greedy = ops.head_score(xd, Wd, t2.to(DEV))
    neg, big = (t2 < 0).to(DEV), (t2 >= vocab).to(DEV)
    assert torch.equal(_bits(lp[neg]), torch.zeros(int(neg.sum()), dtype=torch.int32, device=DEV))      # +0.0 exactly
    assert bool((lp[big] == float("-inf")).all())
    keep = ~(neg | big)
    assert torch.equal(_bits(lp[keep]), _bits(base[0][keep]))
    assert _same((lse, greedy), base[1:])                             # written for every row, whatever its target


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("vocab", [1, 255, 256, 257, 640, 999])
def test_vocab_shorter_than_the_table_is_the_sliced_table(dtype, vocab):
    from quip_amd import ops
    rows, h, table = SHAPES[0]
    x, W, t, *_ = _case(rows, h, table, dtype, 0)
    xd, Wd, td = x.to(DEV), W.to(DEV), t.to(DEV)                      # targets up to 999: some lie at or past `vocab`
    got = ops.head_score(xd, Wd, td, vocab=vocab)
    want = ops.head_score(xd, Wd[:vocab].clone(), td)
    assert _same(got, want)
    assert bool((got[2] < vocab).all())


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_rows_split_over_calls_and_repeated_calls_give_the_same_bits(dtype):
    from quip_amd import ops
    rows, h, vocab = SHAPES[0]
    x, W, t, *_ = _case(rows, h, vocab, dtype, 0)
    xd, Wd, td = x.to(DEV), W.to(DEV), t.to(DEV)
    whole = ops.head_score(xd, Wd, td)
    assert _same(ops.head_score(xd, Wd, td), whole)
    parts = [ops.head_score(xd[a:b], Wd, td[a:b].clone()) for a, b in ((0, 50), (50, 67), (67, 200))]
    assert _same([torch.cat(c) for c in zip(*parts)], whole)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_strided_x_is_the_contiguous_call(dtype):
    from quip_amd import ops
    rows, h, vocab = SHAPES[5]
    x, W, t, *_ = _case(rows, h, vocab, dtype, 5)
    wide = torch.randn(rows, h + 72, generator=torch.Generator().manual_seed(1)).to(dtype)
    wide[:, 8:8 + h] = x
    wide = wide.to(DEV)
    win = wide[:, 8:8 + h]
    assert win.stride(0) == h + 72 and not win.is_contiguous()
    Wd, td = W.to(DEV), t.to(DEV)
    assert _same(ops.head_score(win, Wd, td), ops.head_score(x.to(DEV), Wd, td))


def test_out_and_workspace_are_used_when_given():
    from quip_amd import ops
    rows, h, vocab = SHAPES[1]
    x, W, t, *_ = _case(rows, h, vocab, F16, 1)
    xd, Wd, td = x.to(DEV), W.to(DEV), t.to(DEV)
    want = ops.head_score(xd, Wd, td)
    out = (torch.empty(rows, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, dtype=torch.int64, device=DEV))
    ws = ops.head_score_workspace(rows, vocab, DEV)
    got = ops.head_score(xd, Wd, td, out=out, workspace=ws)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out)) and _same(got, want)
    with pytest.raises(Exception, match="workspace"):
        ops.head_score(xd, Wd, td, workspace=ws[:64])
