"""CPU-side checks of the scoring path: the fifth ABI table (include/quip_amd_score.h <-> _lib.SCORE_SIGNATURES <-> the library's
exports), quipamd_head_score's refusals before any device is touched, and decode.collate_requests against a restatement, in this file's
own words, of how the reference's zero-shot harness batches (context, continuation) requests."""
import ctypes
import os
import re

import pytest
import torch

from quip_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)     # non-null dummy pointers are never dereferenced: the checks come first


def _declared():
    hdr = open(os.path.join(ROOT, "include", "quip_amd_score.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(quipamd_[a-z0-9_]+)\s*\(", hdr)))


def test_every_score_symbol_is_declared_exported_and_bound():
    names = _declared()
    assert names == ["quipamd_head_score", "quipamd_head_score_workspace_bytes"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/quip_amd_score.h but not exported"
    assert sorted(_lib.SCORE_SIGNATURES) == names
    bound = _lib.load()
    for n in names:
        assert getattr(bound, n).argtypes == _lib.SCORE_SIGNATURES[n]
    assert bound.quipamd_head_score_workspace_bytes.restype is ctypes.c_int64
    assert bound.quipamd_head_score.restype is ctypes.c_int


def test_the_score_table_is_disjoint_from_the_other_four():
    for other in (_lib.SIGNATURES, _lib.PREFILL_SIGNATURES, _lib.SAMPLE_SIGNATURES, _lib.GENERATE_SIGNATURES):
        assert not set(_lib.SCORE_SIGNATURES) & set(other)
    for hdr in ("quip_amd.h", "quip_amd_prefill.h", "quip_amd_sample.h", "quip_amd_generate.h"):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        assert not [n for n in _lib.SCORE_SIGNATURES if n in text], hdr


def test_workspace_bytes_follow_the_slices_of_the_vocabulary():
    wb = _lib.load().quipamd_head_score_workspace_bytes
    assert wb(1, 1) == 20 and wb(1, 256) == 20 and wb(1, 257) == 40             # five 4-byte fields per (slice of 256, row)
    assert wb(2048, 50272) == 197 * 2048 * 20
    assert wb(7, 1000) == 7 * wb(1, 1000)                                       # the cut depends on vocab alone
    assert wb(0, 1000) == 0 and wb(5, 0) == 0 and wb(-1, 5) == 0 and wb(5, 65535 * 256 + 1) == 0


def _call(x=ONE, W=ONE, targets=ONE, logprob=ONE, lse=ONE, greedy=ONE, ws=ONE, dtype=1, rows=4, h=64, vocab=100, ldx=None, ldw=None,
          ws_bytes=1 << 20):
    _lib.call("quipamd_head_score", x, h if ldx is None else ldx, W, h if ldw is None else ldw, targets, dtype, rows, h, vocab, logprob, lse,
              greedy, ws, ws_bytes, NULL)


def test_head_score_refuses_bad_arguments_without_a_device():
    for name in ("x", "W", "targets", "logprob", "lse", "greedy", "ws"):
        with pytest.raises(_lib.QuipAmdError, match="null pointer") as e:
            _call(**{name: NULL})
        assert "code 1" in str(e.value)                                         # QUIPAMD_ERR_ARG
    for dtype in (0, 3, -1):
        with pytest.raises(_lib.QuipAmdError, match="f16 / bf16 only") as e:
            _call(dtype=dtype)
        assert "code 4" in str(e.value)                                         # QUIPAMD_ERR_UNSUPPORTED
    for rows in (0, -2):
        with pytest.raises(_lib.QuipAmdError, match="at least one row") as e:
            _call(rows=rows)
        assert "code 2" in str(e.value)                                         # QUIPAMD_ERR_SHAPE
    for vocab in (0, -1, 65535 * 256 + 1):
        with pytest.raises(_lib.QuipAmdError, match="head_score: vocab"):
            _call(vocab=vocab, ws_bytes=1 << 40)
    for h in (0, 16, 48, 100):
        with pytest.raises(_lib.QuipAmdError, match="not a multiple of 32"):
            _call(h=h, ldx=128, ldw=128)
    for kw in (dict(ldx=68), dict(ldw=68), dict(ldx=56), dict(ldw=32)):          # not a multiple of 8; shorter than a row
        with pytest.raises(_lib.QuipAmdError, match="row strides"):
            _call(**kw)
    for name in ("x", "W", "targets", "logprob", "lse", "greedy", "ws"):
        with pytest.raises(_lib.QuipAmdError, match="16-byte aligned"):
            _call(**{name: ctypes.c_void_p(24)})
    with pytest.raises(_lib.QuipAmdError, match="workspace of 79 bytes is too small \\(80 needed\\)"):
        _call(ws_bytes=79)                                                      # 4 rows x 1 slice x 20 bytes


def test_ops_head_score_refuses_cpu_tensors():
    from quip_amd import ops
    x, W, t = torch.ones(4, 64, dtype=torch.float16), torch.ones(100, 64, dtype=torch.float16), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.head_score(x, W, t)
    assert callable(ops.head_score_workspace)


def test_engine_scoring_api_is_there():
    import inspect
    from quip_amd import decode
    for name in ("score", "loglikelihood", "perplexity"):
        assert callable(getattr(decode.DecodeEngine, name))
    assert callable(decode.loglikelihood) and callable(decode.collate_requests)
    for cls in (decode.OPTDecoder, decode.LlamaDecoder):
        p = inspect.signature(cls.prefill).parameters
        assert p["hidden"].default is False and p["all_logits"].default is False
    assert inspect.signature(decode.DecodeEngine.perplexity).parameters["fused"].default is False
    assert inspect.signature(decode.perplexity).parameters["fused"].default is False
    assert inspect.signature(decode.loglikelihood).parameters["bs"].default == 1


# ---- collate_requests ----------------------------------------------------------------------------------------------------------------------
def _harness_batches(requests, bs, max_len):
    """how the zero-shot harness batches, restated: sort by (-total length, tokens), walk in groups of bs; per request the model sees
    the last max_len + 1 tokens of context + continuation without the final one, zero-padded on the right to the FIRST request of the
    group; the continuation is scored on the last len(cont) positions of the unpadded input.  Returns per group a list of
    (request index, padded input, first scored position, continuation)."""
    order = sorted(range(len(requests)), key=lambda i: (-len(requests[i][0] + requests[i][1]), tuple(requests[i][0] + requests[i][1])))
    groups = []
    for lo in range(0, len(order), bs):
        pad_to, rows = None, []
        for i in order[lo:lo + bs]:
            ctx, cont = requests[i]
            assert len(ctx) > 0 and len(cont) > 0 and len(cont) <= max_len
            inp = (ctx + cont)[-(max_len + 1):][:-1]
            pad_to = len(inp) if pad_to is None else pad_to
            rows.append((i, inp + [0] * (pad_to - len(inp)), len(inp) - len(cont), cont))
        groups.append(rows)
    return groups


REQUESTS = [([5, 6, 7], [8, 9]),                       # 0
            ([5, 6, 7], [8, 3]),                       # 1: same length as 0, sorts before it by tokens
            ([1], [2]),                                # 2: the shortest
            (list(range(10, 22)), [3, 4, 5]),          # 3: 15 tokens, longer than max_len + 1 = 9: cut from the left
            ([5, 6, 7], [8, 9]),                       # 4: identical to 0
            ([9, 9, 9, 9], [1]),                       # 5: same length as 0 / 1 / 4
            ([2, 3], [4, 5, 6, 7, 8, 9, 1, 2])]        # 6: a continuation of exactly max_len tokens


@pytest.mark.parametrize("bs", [1, 2, 3, 4, 8])
def test_collate_requests_is_the_harness_batching(bs):
    from quip_amd import decode
    max_len = 8
    got = decode.collate_requests(REQUESTS, bs, max_len)
    want = _harness_batches(REQUESTS, bs, max_len)
    assert len(got) == len(want) == -(-len(REQUESTS) // bs)
    seen = []
    for b, rows in zip(got, want):
        n = len(rows[0][1])
        assert b.ids.dtype == b.targets.dtype == torch.int64 and tuple(b.ids.shape) == tuple(b.targets.shape) == (bs, n)
        assert b.real == len(rows) and len(b.index) == bs
        for r, (i, inp, first, cont) in enumerate(rows):
            assert b.index[r] == i and b.ids[r].tolist() == inp
            tg = [-1] * n
            tg[first:first + len(cont)] = cont
            assert b.targets[r].tolist() == tg                                   # targets on the continuation's positions only
        for r in range(b.real, bs):                                              # a short last batch: copies of its first request
            assert b.index[r] == b.index[0] and torch.equal(b.ids[r], b.ids[0]) and torch.equal(b.targets[r], b.targets[0])
        seen += b.index[:b.real]
    assert sorted(seen) == list(range(len(REQUESTS)))                            # every request once: the caller restores the order
    assert n <= max_len


def test_collate_requests_order_truncation_and_padding_by_hand():
    from quip_amd import decode
    b0, b1, b2, b3 = decode.collate_requests(REQUESTS, 2, 8)
    assert b0.index == [3, 6] and b1.index == [1, 0] and b2.index == [4, 5] and b3.index == [2, 2] and b3.real == 1      # 0 before its twin 4
    assert b0.ids.tolist() == [[16, 17, 18, 19, 20, 21, 3, 4], [3, 4, 5, 6, 7, 8, 9, 1]]       # 15 tokens -> the last 9 without the final one
    assert b0.targets.tolist() == [[-1, -1, -1, -1, -1, 3, 4, 5], [4, 5, 6, 7, 8, 9, 1, 2]]       # a continuation of max_len tokens fills the input
    assert b1.ids.tolist() == [[5, 6, 7, 8], [5, 6, 7, 8]] and b1.targets.tolist() == [[-1, -1, 8, 3], [-1, -1, 8, 9]]
    assert b2.ids.tolist() == [[5, 6, 7, 8], [9, 9, 9, 9]] and b2.targets.tolist() == [[-1, -1, 8, 9], [-1, -1, -1, 1]]
    assert b3.ids.tolist() == [[1], [1]] and b3.targets.tolist() == [[2], [2]]
    padded = decode.collate_requests([([1, 2, 3, 4], [5, 6]), ([7], [8])], 2, 8)[0]
    assert padded.ids.tolist() == [[1, 2, 3, 4, 5], [7, 0, 0, 0, 0]] and padded.targets.tolist() == [[-1, -1, -1, 5, 6], [8, -1, -1, -1, -1]]


def test_collate_requests_refuses_what_the_harness_asserts():
    from quip_amd import decode
    with pytest.raises(ValueError, match="more than max_len 8"):
        decode.collate_requests(REQUESTS + [([1], list(range(9)))], 2, 8)
    with pytest.raises(ValueError, match="empty"):
        decode.collate_requests([([], [1])], 2, 8)
    with pytest.raises(ValueError, match="empty"):
        decode.collate_requests([([1], [])], 2, 8)
    assert decode.collate_requests([], 2, 8) == []
