"""-m gpu: ops.sample_rows (quipamd_sample_rows, csrc/decode_sample.hip) against the fp64 restatement of its contract in
tests/sample_ref.py: greedy == argmax_rows, the Philox wiring exactly, every draw of the sharp inputs acceptable to the oracle (with kept_n,
kept_mass and logprob), ties at the cuts by index, -inf entries, the distribution over 8192 rows, reproducibility and bad rows.

Inputs sit in buffers filled with +inf around and between the rows (row stride n or n + 3, base pointer offset by 0 or 1 element): an
entry read outside a row is the row's maximum and shows up as a wrong token."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sample_ref as R  # noqa: E402

INF = float("inf")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
NS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4096, 32000, 50272, 131072]


def _place(x, ld, off):
    """x [rows, n] copied into a +inf-filled buffer with row stride ld, starting `off` elements behind an aligned address"""
    rows, n = x.shape
    flat = torch.full((off + rows * ld + 16,), INF, dtype=x.dtype, device=DEV)
    view = flat[off:off + rows * ld].view(rows, ld)[:, :n]
    view.copy_(x)
    return view


def _counter(c):
    return torch.tensor([c], dtype=torch.int64, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. greedy
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_greedy_is_argmax_rows(dtype):
    from quip_amd import ops
    ctr = _counter(3)
    greedy = [ops.sample_params(0.0, seed=1, device=DEV), ops.sample_params(0.7, top_k=1, seed=2, device=DEV),
              ops.sample_params(0.0, top_k=40, top_p=0.5, device=DEV)]
    done = 0
    for n in NS:
        g = torch.Generator().manual_seed(n)
        x = torch.randint(-6, 7, (16, n), generator=g).to(dtype)              # small integers: the maximum repeats in most rows
        x[1] = x[1, 0]                                                       # a constant row: the answer is index 0
        for rows in (1, 3, 16):
            for ld in (n, n + 3):
                for off in (0, 1):
                    v = _place(x[:rows].to(DEV), ld, off)
                    want = ops.argmax_rows(v)
                    assert torch.equal(want.cpu(), x[:rows].float().argmax(-1)) or n > 1     # (torch.argmax also takes the first maximum)
                    for p in greedy:
                        out, lp, kn, km = ops.sample_rows(v, p, ctr)
                        assert torch.equal(out, want), (n, rows, ld, off)
                        assert not lp.any() and bool((kn == 1).all()) and bool((km == 1).all())
                        done += 1
    assert done == len(NS) * 3 * 2 * 2 * 3


# ---------------------------------------------------------------------------------------------------------------- 2. Philox wiring
def test_philox_wiring_is_exact_on_equal_logits():
    """n = 4096 equal logits: every weight is 1, every sum an exact integer, so out == floor(u * 4096) with nothing tolerated"""
    from quip_amd import ops
    n, rows = 4096, 16
    counters = list(range(63)) + [(1 << 32) + 5]
    x = torch.zeros(rows, n, dtype=torch.float16, device=DEV)
    ctr = _counter(0)
    for seed in (12345, (0xDEADBEEF << 32) | 0x1357):
        p = ops.sample_params(1.0, seed=seed, device=DEV)
        outs, lps = [], []
        for c in counters:
            ctr.fill_(c)
            out, lp, kn, km = ops.sample_rows(x, p, ctr)
            outs.append(out)
            lps.append(lp)
        got = torch.stack(outs).cpu().numpy()
        want = np.floor(R.uniforms(seed, counters, np.arange(rows)) * n).astype(np.int64)
        assert np.array_equal(got, want)
        assert want.min() >= 0 and want.max() < n and len(np.unique(want)) > 500
        assert np.allclose(torch.stack(lps).cpu().numpy(), np.log(1.0 / n), atol=1e-6) and bool((kn == n).all()) and bool((km == 1).all())


# ---------------------------------------------------------------------------------------------------------------- 3. draws against the oracle
_ORACLES = {}


def _oracle(case):
    if case not in _ORACLES:
        n, scale, T, k, p, dt = case
        x = R.make_logits(n, scale, dt)
        _ORACLES[case] = (x, R.Oracle(R.values(x), T, k, p))
    return _ORACLES[case]


def _run_case(case, aligned):
    from quip_amd import ops
    n, scale, T, k, p, dt = case
    x, o = _oracle(case)
    v = _place(x[None].expand(R.ROWS, n).to(DEV), n if aligned else n + 3, 0 if aligned else 1)
    params = ops.sample_params(T, top_k=k, top_p=p, seed=R.SEED, device=DEV)
    ctr = _counter(0)
    res = []
    for c in range(R.COUNTERS):
        ctr.fill_(R.COUNTER0 + c)
        res.append(ops.sample_rows(v, params, ctr))
    out, lp, kn, km = (torch.stack([r[i] for r in res]).cpu().numpy().ravel() for i in range(4))
    u = R.uniforms(R.SEED, R.COUNTER0 + np.arange(R.COUNTERS), np.arange(R.ROWS)).ravel()
    return o, u, out, lp, kn, km


@pytest.mark.parametrize("ci", range(len(R.SHARP)), ids=lambda i: "-".join(str(v) for v in R.SHARP[i]))
def test_every_draw_is_acceptable_to_the_oracle(ci):
    case = R.SHARP[ci]
    n, scale, T, k, p, dt = case
    o, u, out, lp, kn, km = _run_case(case, aligned=ci % 2 == 0)
    assert out.min() >= 0 and out.max() < n
    ok = o.accepts(u, out)
    exact = out == o.draw(u)
    print(f"{case}: {int(ok.sum())} of {ok.size} draws acceptable, {int(exact.sum())} equal to the fp64 draw; kept_n {kn.min()}..{kn.max()} "
          f"(oracle {o.kept_n} in [{o.n_lo}, {o.n_hi}]); kept_mass {km.min():.6f}..{km.max():.6f} (oracle {o.kept_mass:.6f}); "
          f"max |logprob - oracle| {np.abs(lp - o.logprob(out))[ok].max():.2e}")
    assert ok.all(), (case, np.nonzero(~ok)[0][:8], out[~ok][:8], o.draw(u)[~ok][:8])
    assert (kn >= o.n_lo).all() and (kn <= o.n_hi).all()
    want_mass = np.array([o.mass_of(c) for c in kn]) if p < 1.0 else np.ones_like(km)
    assert np.abs(km - want_mass).max() <= (R.EPS if p < 1.0 else 0.0)
    assert np.abs(lp - o.logprob(out)).max() <= 1e-3


def test_flat_input_validity_and_kept_n_sandwich():
    n = R.FLAT[0]
    o, u, out, lp, kn, km = _run_case(R.FLAT, aligned=True)
    print(f"flat: kept_n {kn.min()}..{kn.max()} (oracle {o.kept_n} in [{o.n_lo}, {o.n_hi}]), {int(o.accepts(u, out).sum())} of {out.size} acceptable")
    assert out.min() >= 0 and out.max() < n
    assert (kn >= o.n_lo).all() and (kn <= o.n_hi).all()
    assert np.isfinite(lp).all() and (lp < 0).all()


# ---------------------------------------------------------------------------------------------------------------- 4. ties at the cut
def _survivors_seen(x, T, k, p, dtype, draws=256):
    """(kept_n of every draw, the set of tokens 256 draws returned) for one row x"""
    from quip_amd import ops
    v = _place(torch.tensor([x], dtype=dtype).expand(draws, len(x)).to(DEV), len(x) + 3, 1)
    out, lp, kn, km = ops.sample_rows(v, ops.sample_params(T, top_k=k, top_p=p, seed=99, device=DEV), _counter(17))
    return kn.cpu().numpy(), set(out.cpu().tolist()), km.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_ties_at_the_cuts_go_to_the_smaller_indices(dtype):
    # top-p on equal logits: p = 1/16 each, entry j has j/16 in front of it -- exact in fp32 and in the kernel's integers
    kn, seen, km = _survivors_seen([0.0] * 16, 1.0, 0, 0.5, dtype)
    assert (kn == 8).all() and seen == set(range(8)) and (km == 0.5).all()
    kn, seen, km = _survivors_seen([2.0] * 64, 0.5, 0, 0.25, dtype)
    assert (kn == 16).all() and seen == set(range(16)) and (km == 0.25).all()
    kn, seen, km = _survivors_seen([2.0] * 64, 0.5, 40, 0.25, dtype)            # top-k 40 first: p = 1/40, j/40 < 0.25 for j < 10
    assert (kn == 10).all() and seen == set(range(10)) and (km == 0.25).all()
    # top-k across a tie: four entries share the maximum, k = 2 and k = 3 take the first ones; -1 entries never
    row = [-1.0, 3.0, -1.0, 3.0, 3.0, -1.0, 3.0, -1.0]
    for k, want in ((2, {1, 3}), (3, {1, 3, 4}), (4, {1, 3, 4, 6})):
        kn, seen, km = _survivors_seen(row, 1.0, k, 1.0, dtype)
        assert (kn == k).all() and seen == want and (km == 1.0).all()
    kn, seen, _ = _survivors_seen(row, 1.0, 6, 1.0, dtype)                       # ... and the cut inside the lower tie
    assert (kn == 6).all() and seen == {1, 3, 4, 6, 0, 2}
    # top-p across a tie of unequal groups: 3.0 x 4 hold 0.9820 of the mass, 0.2455 each -- 0.6 cuts after three of them (0.491 < 0.6 <= 0.7365)
    kn, seen, _ = _survivors_seen(row, 1.0, 0, 0.6, dtype)
    assert (kn == 3).all() and seen == {1, 3, 4}
    kn, seen, _ = _survivors_seen(row, 1.0, 0, 0.99, dtype)                      # 0.9820 + 0.0045 j < 0.99 for j < 2: two of the four -1 entries
    assert (kn == 6).all() and seen == {1, 3, 4, 6, 0, 2}
    # 64 entries, the tie group spread over a segment boundary of the kernel's index order is covered by n = 1025 below
    big = [0.0] * 1025
    for i in (5, 600, 1024):
        big[i] = 4.0
    kn, seen, _ = _survivors_seen(big, 1.0, 2, 1.0, dtype)
    assert (kn == 2).all() and seen == {5, 600}


# ---------------------------------------------------------------------------------------------------------------- 5. -inf
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_minus_inf_entries_are_never_returned(dtype):
    from quip_amd import ops
    n, rows = 1025, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, n, generator=g).to(dtype)
    dead = torch.rand(rows, n, generator=g) < 0.7
    dead[:, 7] = False
    x[dead] = -INF
    v = _place(x.to(DEV), n + 3, 1)
    for T, k, p in ((1.0, 0, 1.0), (2.0, 900, 1.0), (1.5, 0, 0.999), (1.0, 600, 0.9)):
        out, lp, kn, km = ops.sample_rows(v, ops.sample_params(T, top_k=k, top_p=p, seed=3, device=DEV), _counter(2))
        out = out.cpu()
        assert not dead[torch.arange(rows), out].any(), (T, k, p)
        assert bool((kn.cpu() <= (~dead).sum(1)).all()) and bool((kn > 0).all())
    one = torch.full((3, n), -INF, dtype=dtype)
    one[0, 0], one[1, 512], one[2, n - 1] = 1.5, -3.0, 0.0
    out, lp, kn, km = ops.sample_rows(_place(one.to(DEV), n, 0), ops.sample_params(0.9, top_p=0.8, seed=4, device=DEV), _counter(0))
    assert out.tolist() == [0, 512, n - 1] and lp.tolist() == [0.0, 0.0, 0.0] and kn.tolist() == [1, 1, 1] and km.tolist() == [1.0, 1.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------- 6. distribution
def test_distribution_over_8192_rows():
    import scipy.stats
    from quip_amd import ops
    n, rows = 64, 8192
    x = (1.5 * torch.randn(n, generator=torch.Generator().manual_seed(64))).to(torch.float16)
    o = R.Oracle(R.values(x), 0.9)
    v = x[None].expand(rows, n).contiguous().to(DEV)
    seed, c = 2024, 77
    out, lp, kn, km = ops.sample_rows(v, ops.sample_params(0.9, seed=seed, device=DEV), _counter(c))
    out = out.cpu().numpy()
    assert out.min() >= 0 and out.max() < n
    expect = o.prob * rows

    def pearson(tokens):
        return float((((np.bincount(tokens, minlength=n) - expect) ** 2) / expect).sum())
    u = R.uniforms(seed, [c], np.arange(rows)).ravel()
    stat, own = pearson(out), pearson(o.draw(u))
    bound = float(scipy.stats.chi2.ppf(1 - 1e-6, n - 1))
    print(f"Pearson statistic over {rows} rows: kernel {stat:.1f}, the oracle's own draws {own:.1f}, bound {bound:.1f}; "
          f"{int((out == o.draw(u)).sum())} of {rows} tokens equal the fp64 draws")
    assert stat < bound
    assert o.accepts(u, out).all()


# ---------------------------------------------------------------------------------------------------------------- 7. reproducibility
def test_the_same_call_gives_the_same_bits():
    from quip_amd import ops
    import guard_arena as G
    n, rows = 50272, 16
    x = (4 * torch.randn(rows, n, generator=torch.Generator().manual_seed(7))).to(torch.float16).to(DEV)
    ctr = _counter(123456789012)
    for T, k, p in ((0.8, 50, 0.9), (1.0, 0, 0.95), (1.3, 0, 1.0), (0.7, 2000, 1.0)):
        params = ops.sample_params(T, top_k=k, top_p=p, seed=5, device=DEV)
        runs = [ops.sample_rows(x, params, ctr) for _ in range(3)]
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert G.bit_equal(a, b)
        assert len(set(runs[0][0].tolist())) > 1


def test_the_parameters_are_read_at_run_time():
    from quip_amd import ops
    n, rows = 4096, 16
    x = (3 * torch.randn(rows, n, generator=torch.Generator().manual_seed(8))).to(torch.bfloat16).to(DEV)
    ctr = _counter(9)
    params = ops.sample_params(1.0, seed=1, device=DEV)
    a = ops.sample_rows(x, params, ctr)[0].clone()
    ops.write_sample_params(params, 1.0, seed=2)
    b = ops.sample_rows(x, params, ctr)[0].clone()
    ops.write_sample_params(params, 1.0, top_k=1, seed=2)
    c = ops.sample_rows(x, params, ctr)[0].clone()
    ops.write_sample_params(params, 1.0, seed=1)
    d = ops.sample_rows(x, params, ctr)[0].clone()
    ctr.fill_(10)
    e = ops.sample_rows(x, params, ctr)[0].clone()
    assert not torch.equal(a, b) and torch.equal(c, ops.argmax_rows(x)) and torch.equal(a, d) and not torch.equal(a, e)


# ---------------------------------------------------------------------------------------------------------------- 8. bad rows
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_bad_rows_yield_a_token_in_range_and_leave_their_neighbours_alone(dtype):
    from quip_amd import ops
    import guard_arena as G
    n, rows = 1025, 7
    good = (3 * torch.randn(rows, n, generator=torch.Generator().manual_seed(11))).to(dtype)
    bad = good.clone()
    bad[1] = float("nan")
    bad[3] = -INF
    bad[5, 700] = INF
    for T, k, p in ((1.0, 0, 1.0), (0.8, 50, 0.9), (1.0, 0, 0.5), (0.0, 0, 1.0)):
        params = ops.sample_params(T, top_k=k, top_p=p, seed=6, device=DEV)
        ctr = _counter(4)
        ref = ops.sample_rows(_place(good.to(DEV), n + 3, 1), params, ctr)
        got = ops.sample_rows(_place(bad.to(DEV), n + 3, 1), params, ctr)
        torch.cuda.synchronize()                                             # the call returns
        assert bool((got[0] >= 0).all()) and bool((got[0] < n).all())
        for a, b in zip(ref, got):
            assert G.bit_equal(a[0::2], b[0::2]), (T, k, p)                  # rows 0, 2, 4, 6 are the same rows in both calls
