"""What ops.generate_rows adds to ops.sample_rows (include/quip_amd_generate.h), restated: the repetition penalty in numpy fp32 and the stop /
done bookkeeping in plain Python.  A helper of tests/test_generate_host.py and tests/test_gpu_generate*.py, not a test; the sampling itself
is tests/sample_ref.py's, imported as it is.

The GPU tests hold the kernel to ops.sample_rows run on penalise(float(logits), history, p): the kernel penalises in fp32 as it loads and
ops.sample_rows reads fp32, so the two see the same numbers and agree bit for bit -- nothing is tolerated."""
import numpy as np

import sample_ref as R  # noqa: F401  (re-exported: the oracle, Philox, the test inputs)


def penalise(vals_fp32, hist_row, p):
    """Hugging Face's RepetitionPenaltyLogitsProcessor on one row, fp32: for every DISTINCT id of hist_row inside [0, n) the logit x becomes
    x < 0 ? x * p : x / p (an IEEE division); ids outside the vocabulary are ignored.  Returns a new float32 array."""
    x = np.array(vals_fp32, dtype=np.float32, copy=True)
    assert x.ndim == 1
    ids = np.unique(np.asarray(hist_row, dtype=np.int64))
    ids = ids[(ids >= 0) & (ids < x.shape[0])]
    p32 = np.float32(p)
    sel = x[ids]
    with np.errstate(invalid="ignore", over="ignore"):
        x[ids] = np.where(sel < 0, sel * p32, sel / p32).astype(np.float32)
    return x


def penalise_rows(vals_fp32, hist, lengths, ps):
    """penalise() per row: vals [rows, n] fp32, hist [rows, cap], the first lengths[r] positions of row r count, ps[r] its penalty"""
    return np.stack([penalise(vals_fp32[r], hist[r, :lengths[r]], ps[r]) for r in range(vals_fp32.shape[0])])


def stop_step(tokens, done, stop_pos, stop_ids, counter, pad_id):
    """one launch's bookkeeping.  tokens: what the rows would draw (a plain launch's answer); done / stop_pos: the state on entry (lists).
    Returns (out, done, stop_pos) after the launch: a row done on entry yields pad_id and keeps its state, any other row yields its token
    and, when that is a stop id, becomes done with stop_pos = counter."""
    out, d2, s2 = [], list(done), list(stop_pos)
    for r, t in enumerate(tokens):
        if done[r]:
            out.append(pad_id)
            continue
        out.append(int(t))
        if int(t) in stop_ids:
            d2[r], s2[r] = 1, counter
    return out, d2, s2


def trim(plain, stop_ids, pad_id):
    """the whole continuation: plain [n][bs] tokens of a run without stops (list of lists or array).  Returns (tokens [n'][bs], lengths [bs],
    first_stop [bs] (step index, or None)): each sequence equals the plain run up to and including its first stop token, pad_id behind it;
    n' is the latest stop's step + 1 when every sequence stopped, else n."""
    plain = np.asarray(plain)
    n, bs = plain.shape
    first = []
    for b in range(bs):
        hits = [i for i in range(n) if int(plain[i, b]) in stop_ids]
        first.append(hits[0] if hits else None)
    n_out = max(first) + 1 if bs and all(f is not None for f in first) else n
    toks = plain[:n_out].copy()
    for b, f in enumerate(first):
        if f is not None:
            toks[f + 1:, b] = pad_id
    lengths = [f + 1 if f is not None else n_out for f in first]
    return toks, lengths, first
