"""-m gpu: ops.generate_rows (quipamd_generate_rows, csrc/decode_generate.hip) held to ops.sample_rows BIT FOR BIT -- the two launches run
one copy of the sampling arithmetic (csrc/sample_body.h), sums are integers and the draw is Philox(seed; counter, row), so nothing is
tolerated anywhere in this file:

  identity    penalty 1, no history, no stops, equal parameters in every row: the four outputs of ops.sample_rows
  penalty     == ops.sample_rows on the fp32 tensor generate_ref.penalise(float(logits), history, p): the kernel penalises in fp32 as it
              loads, ops.sample_rows reads fp32; `logits` keeps its bits
  per row     row r of a launch with four parameter sets == row r of the launch that gives every row set r
  stop        done / stop_pos as generate_ref.stop_step says, finished rows yield pad_id, running rows are their plain selves
  history     hist[r, c - 1] = fed[r], hist[r, c] = out[r], nothing outside [0, cap), with fed aliasing out as well
  and the same call twice gives the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import generate_ref as GR  # noqa: E402
import guard_arena as G  # noqa: E402
from test_gpu_sample_contract import PATHS  # noqa: E402

INF = float("inf")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
NAMES = ("out", "logprob", "kept_n", "kept_mass")
SEED = 0x5EED5EED12345678


def _place(x, ld, off):
    """x [rows, n] copied into a +inf-filled buffer with row stride ld, starting `off` elements behind an aligned address: an entry read
    outside a row would be the row's maximum"""
    rows, n = x.shape
    flat = torch.full((off + rows * ld + 16,), INF, dtype=x.dtype, device=DEV)
    view = flat[off:off + rows * ld].view(rows, ld)[:, :n]
    view.copy_(x)
    return view


def _counter(c):
    return torch.tensor([c], dtype=torch.int64, device=DEV)


def _gparams(rows, T=1.0, k=0, p=1.0, seed=SEED, pen=1.0):
    from quip_amd import ops
    return ops.write_generate_params(ops.generate_params(rows, device=DEV), None, T, k, p, seed, pen)


def _same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        assert G.bit_equal(a, b), (what, name, a.tolist()[:8], b.tolist()[:8])


def _logits(rows, n, dtype, seed):
    """4 * randn with exact zeros, a -0, runs of -inf and equal values sprinkled in (no NaN: bad rows are added where a test wants them)"""
    g = torch.Generator().manual_seed(seed)
    x = 4 * torch.randn(rows, n, generator=g)
    if n >= 64:
        pick = torch.randint(0, n, (rows, 24), generator=g)
        for r in range(rows):
            x[r, pick[r, :8]] = 0.0
            x[r, pick[r, 8:16]] = -INF
            x[r, pick[r, 16:20]] = 2.5
            x[r, pick[r, 20]] = -0.0
    return x.to(dtype)


# ---------------------------------------------------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_without_penalty_history_and_stops_it_is_sample_rows_bit_for_bit(dtype):
    from quip_amd import ops
    done = 0
    for n in (1, 7, 511, 512, 513, 4099, 50272, 262144):
        x = _logits(5, n, dtype, n)
        for rows in (1, 5):
            for ld, off in ((n, 0), (n + 3, 1)):                             # 16-byte aligned rows, and rows on odd element addresses
                v = _place(x[:rows].to(DEV), ld, off)
                ctr = _counter(1000 + n)
                for T, k, p in PATHS:
                    want = ops.sample_rows(v, ops.sample_params(T, top_k=k, top_p=p, seed=SEED, device=DEV), ctr)
                    got = ops.generate_rows(v, _gparams(rows, T, k, p, SEED), ctr)
                    _same(got, want, (n, rows, ld, T, k, p))
                    done += 1
                if n in (513, 50272):                                        # a history that is there but not used: penalty 1; nothing to read
                    T, k, p = PATHS[4]
                    want = ops.sample_rows(v, ops.sample_params(T, top_k=k, top_p=p, seed=SEED, device=DEV), ctr)
                    hist = torch.randint(0, n, (rows, 32), generator=torch.Generator().manual_seed(n + ld)).to(torch.int32).to(DEV)
                    _same(ops.generate_rows(v, _gparams(rows, T, k, p, SEED, pen=1.0), ctr, hist=hist.clone()), want, "penalty 1")
                    zero = _counter(0)
                    want0 = ops.sample_rows(v, ops.sample_params(T, top_k=k, top_p=p, seed=SEED, device=DEV), zero)
                    _same(ops.generate_rows(v, _gparams(rows, T, k, p, SEED, pen=1.7), zero, hist=hist.clone()), want0, "empty history")
    assert done == 8 * 2 * 2 * len(PATHS)


# ---------------------------------------------------------------------------------------------------------------- 2. penalty
CAP = 1040
LENGTHS = (0, 1, 63, 64, 65, 1000, CAP)
PEN_PATHS = [(0.0, 0, 1.0), (0.9, 0, 1.0), (0.9, 40, 0.9)]


def _history(x, n):
    """int32 [4, CAP]: row 0 ids all over the place, below 0 and from n up included; row 1 heavy duplicates (16 distinct ids, the row's top
    token among them); row 2 the row's 64 largest logits first (greedy must move) then anything; row 3 (the bad row's) like row 0"""
    g = torch.Generator().manual_seed(n + 1)
    top = x.float().nan_to_num(nan=-INF).topk(min(64, n), dim=1).indices
    h = torch.randint(-5, n + 5, (4, CAP), generator=g)
    few = torch.cat([top[1, :1], torch.randint(0, n, (15,), generator=g)])
    h[1] = few[torch.randint(0, 16, (CAP,), generator=g)]
    h[1, 0] = top[1, 0]
    h[2, :top.shape[1]] = top[2]
    return h.to(torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("n", [513, 50272, 262144])
def test_penalty_is_sample_rows_on_the_penalised_fp32_row(n, dtype):
    from quip_amd import ops
    x = _logits(4, n, dtype, 3 * n)
    x[3, n // 2] = float("nan")                                              # a bad row: the sample contract's behaviour, the same bits
    x[0, :4] = torch.tensor([0.0, -1.5, -INF, 3.0]).to(dtype)
    hist0 = _history(x, n)
    hist0[0, :4] = torch.tensor([0, 1, 2, 3], dtype=torch.int32)             # a zero, a negative, a -inf and a positive entry are penalised
    v = _place(x.to(DEV), *((n + 3, 1) if n == 513 else (n, 0)))               # rows on odd element addresses once, 16-byte loads otherwise
    frozen = G.freeze(logits=v)
    vals = x.float().numpy()
    hist_d = hist0.to(DEV)
    moved = 0
    for c in LENGTHS:
        ctr = _counter(c)
        for pen in (0.5, 1.0, 1.3):
            ref = torch.from_numpy(GR.penalise_rows(vals, hist0.numpy(), [min(c, CAP)] * 4, [pen] * 4)).to(DEV)
            for T, k, p in PEN_PATHS:
                want = ops.sample_rows(ref, ops.sample_params(T, top_k=k, top_p=p, seed=SEED, device=DEV), ctr)
                hist = hist_d.clone()
                got = ops.generate_rows(v, _gparams(4, T, k, p, SEED, pen=pen), ctr, hist=hist)
                _same(got, want, (n, c, pen, T, k, p))
                if T == 0.0 and c and pen != 1.0:
                    plain = ops.sample_rows(v, ops.sample_params(0.0, device=DEV), ctr)[0]
                    moved += int((plain != got[0]).sum())
    torch.cuda.synchronize()
    frozen.assert_frozen()                                                   # the logits are penalised on the fly, never written
    assert moved >= 6, "the penalty never changed a greedy token: the histories do not test it"


# ---------------------------------------------------------------------------------------------------------------- 3. per-row parameters
SETS = [(0.9, 40, 0.9, 11, 1.3), (0.0, 0, 1.0, 0, 1.2), (1.3, 0, 1.0, (1 << 63) + 5, 1.0), (0.7, 0, 0.8, 11, 0.6)]


@pytest.mark.parametrize("dtype,n", [(torch.float16, 50272), (torch.bfloat16, 4099), (torch.float32, 513)], ids=str)
def test_every_row_uses_its_own_parameters(dtype, n):
    from quip_amd import ops
    x = _logits(4, n, dtype, 7 * n).to(DEV)
    hist0 = _history(x.cpu(), n).to(DEV)
    ctr = _counter(300)
    mixed = ops.write_generate_params(ops.generate_params(4, device=DEV), None, *[[s[i] for s in SETS] for i in range(5)])
    got = ops.generate_rows(x, mixed, ctr, hist=hist0.clone())
    outs = []
    for r, s in enumerate(SETS):
        uni = ops.generate_rows(x, _gparams(4, *s), ctr, hist=hist0.clone())
        for name, a, b in zip(NAMES, got, uni):
            assert G.bit_equal(a[r:r + 1], b[r:r + 1]), (name, r)
        outs.append(uni[0].clone())
    assert any(not torch.equal(outs[0], o) for o in outs[1:])                # the four sets are four different launches
    one = ops.generate_params(4, device=DEV)                                 # ... and a single row can be rewritten in place
    for r, s in enumerate(SETS):
        ops.write_generate_params(one, r, *s)
    assert torch.equal(one, mixed)
    _same(ops.generate_rows(x, one, ctr, hist=hist0.clone()), got, "row-wise writes")


# ---------------------------------------------------------------------------------------------------------------- 4. stop
@pytest.mark.parametrize("n_stop", [0, 1, 16])
def test_stop_ids_finish_rows_and_finished_rows_yield_pad(n_stop):
    from quip_amd import ops
    n, rows, pad, c = 4099, 6, 3, 20
    x = _logits(rows, n, torch.float16, 99).to(DEV)
    prm = _gparams(rows, 0.9, 40, 0.9, SEED)
    plain1 = [t.clone() for t in ops.generate_rows(x, prm, _counter(c))]
    plain2 = [t.clone() for t in ops.generate_rows(x, prm, _counter(c + 1))]
    t1 = plain1[0].tolist()
    assert len(set(t1[0::2])) == 3 and not set(t1[0::2]) & set(t1[1::2])     # rows 0, 2, 4 can stop while 1, 3, 5 go on
    unused = [i for i in range(n - 40, n) if i not in t1 + plain2[0].tolist()]
    stops = {0: [], 1: [t1[2]], 16: [t1[0], t1[2], t1[4]] + unused[:13]}[n_stop]
    stop_ids = torch.tensor(stops, dtype=torch.int32, device=DEV)
    done = torch.zeros(rows, dtype=torch.int32, device=DEV)
    stop_pos = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
    got1 = ops.generate_rows(x, prm, _counter(c), stop_ids=stop_ids, pad_id=pad, done=done, stop_pos=stop_pos)
    _same(got1, plain1, "first launch: nobody was done")
    want_out, want_done, want_pos = GR.stop_step(t1, [0] * rows, [-1] * rows, set(stops), c, pad)
    assert want_out == t1 and done.tolist() == want_done and stop_pos.tolist() == want_pos
    assert sum(want_done) == {0: 0, 1: 1, 16: 3}[n_stop]
    got2 = ops.generate_rows(x, prm, _counter(c + 1), stop_ids=stop_ids, pad_id=pad, done=done, stop_pos=stop_pos)
    out2, done2, pos2 = GR.stop_step(plain2[0].tolist(), want_done, want_pos, set(stops), c + 1, pad)
    assert got2[0].tolist() == out2 and done.tolist() == done2 and stop_pos.tolist() == pos2
    for r in range(rows):
        if want_done[r]:                                                     # finished in the first launch: pad, and the fixed triple
            assert (got2[0][r].item(), got2[1][r].item(), got2[2][r].item(), got2[3][r].item()) == (pad, 0.0, 0, 1.0)
        else:                                                                # running rows do not see their neighbours
            for name, a, b in zip(NAMES, got2, plain2):
                assert G.bit_equal(a[r:r + 1], b[r:r + 1]), (name, r)
    # done without stop ids, stop ids without done: each part works alone
    only_pos = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
    ops.generate_rows(x, prm, _counter(c), stop_ids=stop_ids if n_stop else None, stop_pos=only_pos)
    assert only_pos.tolist() == want_pos
    all_done = torch.ones(rows, dtype=torch.int32, device=DEV)
    out = ops.generate_rows(x, prm, _counter(c), pad_id=pad, done=all_done)[0]
    assert out.tolist() == [pad] * rows and all_done.tolist() == [1] * rows


# ---------------------------------------------------------------------------------------------------------------- 5. history writes
@pytest.mark.parametrize("alias", [False, True], ids=["fed", "fed_is_out"])
def test_history_cells_and_the_fed_token_counts(alias):
    from quip_amd import ops
    n, rows, cap, ldh = 1025, 5, 24, 29
    x = _logits(rows, n, torch.bfloat16, 5).to(DEV)
    top = x.float().argmax(-1)
    base = torch.randint(0, n, (rows, ldh), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(DEV)
    prm = _gparams(rows, 0.0, pen=1.3)                                       # greedy with a penalty: the fed token must count at once
    for c in (0, 1, 7, cap - 1, cap, cap + 1, cap + 5):
        buf = base.clone()
        hist = buf[:, :cap]                                                  # row stride 29 > cap 24: the columns behind cap are not the kernel's
        fed = top.clone()                                                    # feeding each row's best token: the penalty then moves the argmax
        out = fed if alias else torch.full((rows,), -7, dtype=torch.int64, device=DEV)
        got = ops.generate_rows(x, prm, _counter(c), hist=hist, fed=fed, out=out)
        want_hist = base.clone()
        if 0 <= c - 1 < cap:
            want_hist[:, c - 1] = top.to(torch.int32)
        hl = min(c, cap)
        ref = torch.from_numpy(GR.penalise_rows(x.float().cpu().numpy(), want_hist.cpu().numpy(), [hl] * rows, [1.3] * rows)).to(DEV)
        want = ops.sample_rows(ref, ops.sample_params(0.0, device=DEV), _counter(c))
        _same(got, want, (c, alias))
        if 0 <= c < cap:
            want_hist[:, c] = want[0].to(torch.int32)
        assert torch.equal(buf, want_hist), (c, alias)                       # the two cells, nothing else, nothing outside [0, cap)
        assert got[0] is out
        if 1 <= c <= cap:
            assert bool((got[0] != top).any()), "the token just fed was not penalised"
    quiet = base.clone()                                                     # no fed: only hist[r, c]; no hist: nothing
    got = ops.generate_rows(x, prm, _counter(3), hist=quiet[:, :cap])
    assert torch.equal(quiet[:, :3], base[:, :3]) and torch.equal(quiet[:, 4:], base[:, 4:]) and torch.equal(quiet[:, 3], got[0].to(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 6. determinism
def test_the_same_call_gives_the_same_bits():
    from quip_amd import ops
    n, rows = 50272, 16
    x = _logits(rows, n, torch.float16, 7).to(DEV)
    hist0 = torch.randint(0, n, (rows, 600), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(DEV)
    plain = ops.generate_rows(x, _gparams(rows, 0.8, 50, 0.9, 5), _counter(500))[0].tolist()
    stop_ids = torch.tensor(plain[:4], dtype=torch.int32, device=DEV)
    for T, k, p, pen in ((0.8, 50, 0.9, 1.2), (1.0, 0, 0.95, 1.3), (1.3, 0, 1.0, 0.7), (0.0, 0, 1.0, 1.5)):
        runs = []
        for _ in range(3):
            hist, done = hist0.clone(), torch.zeros(rows, dtype=torch.int32, device=DEV)
            pos = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
            res = ops.generate_rows(x, _gparams(rows, T, k, p, 5, pen), _counter(500), hist=hist, stop_ids=stop_ids, done=done, stop_pos=pos)
            runs.append(list(res) + [hist, done, pos])
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert G.bit_equal(a, b)
        assert len(set(runs[0][0].tolist())) > 1
