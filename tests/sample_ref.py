"""What ops.sample_rows promises (include/quip_amd_sample.h), restated in fp64 -- the oracle of tests/test_sample_host.py and
tests/test_gpu_sample*.py.  A plain module: no fixtures, no GPU.

  philox4x32_10 / uniform      the generator, word for word from the paper (Salmon et al., SC'11), in plain Python integers
  uniforms                     the same for arrays of counters and rows (numpy); the host test checks it against the plain one
  Oracle(values, T, k, p)      order, top-k, top-p, kept_n with its sandwich, the survivors' prefix sums in index order, and per draw the
                               set of ACCEPTABLE tokens: those whose interval [C_(i-1), C_i), widened by delta * Z on both sides, holds u * Z

delta = 3e-5: the kernel's weights are fp32 exp with a hardware exponential (relative error of a weight about 1e-6 for the arguments that
carry mass), its sums are exact integers in 2^-40 fixed point (at most 2^18 truncations of 2^-40: 2.4e-7), so C_i / Z is off by a few 1e-6 at
most; delta is the bound of an fp32 tree of sums (n / 1024 + 20 terms per association: 148 * 2^-24 = 9e-6 at n = 131072) plus the exponential,
times three -- what any implementation of the contract in fp32 can meet.
eps = 1e-4 for the top-p mass is the same bound with room."""
import numpy as np
import torch

DELTA = 3e-5
EPS = 1e-4
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xffffffff


def philox4x32_10(ctr, key):
    """ctr: four 32-bit words, key: two; returns the four output words"""
    c, k = list(ctr), list(key)
    for rnd in range(10):
        if rnd:
            k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
    return c


def uniform(seed, counter, row):
    """the u of (seed, counter, row): key (lo32 seed, hi32 seed), counter words (lo32 counter, hi32 counter, row, 0), first output word"""
    x0 = philox4x32_10([counter & MASK, (counter >> 32) & MASK, row & MASK, 0], [seed & MASK, (seed >> 32) & MASK])[0]
    return (x0 >> 8) * 2.0 ** -24


def uniforms(seed, counters, rows):
    """u for every (counter, row) pair: float64 [len(counters), len(rows)]"""
    ctr = np.asarray(counters, dtype=np.uint64)[:, None]
    rw = np.asarray(rows, dtype=np.uint64)[None, :]
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    c = [np.broadcast_to(ctr & m, (ctr.shape[0], rw.shape[1])).copy(), np.broadcast_to(ctr >> s32, (ctr.shape[0], rw.shape[1])).copy(),
         np.broadcast_to(rw & m, (ctr.shape[0], rw.shape[1])).copy(), np.zeros((ctr.shape[0], rw.shape[1]), dtype=np.uint64)]
    k = [np.uint64(seed & MASK), np.uint64((seed >> 32) & MASK)]
    for rnd in range(10):
        if rnd:
            k = [(k[0] + np.uint64(W0)) & m, (k[1] + np.uint64(W1)) & m]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                  # 32 x 32 bits: inside 64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m, (p0 >> s32) ^ c[3] ^ k[1], p0 & m]
    return (c[0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def make_logits(n, scale, dtype):
    """the test inputs: (scale * randn(n)) rounded to the dtype, RandomState(n + int(10 * scale)); returns the torch tensor [n]"""
    x = (scale * np.random.RandomState(n + int(10 * scale)).randn(n)).astype(np.float32)
    return torch.from_numpy(x).to(TORCH_DT[dtype])


def values(t):
    """a logits tensor's exact values as float64 numpy"""
    return t.detach().cpu().double().numpy()


# (n, scale, temperature, top_k, top_p, dtype): the inputs on which every draw is compared with the oracle
SHARP = [(1000, 6, 1.0, 0, 1.0, "bf16"), (32000, 6, 1.0, 0, 1.0, "f16"), (50272, 6, 1.0, 0, 1.0, "f16"), (131072, 6, 1.0, 0, 1.0, "f16"),
         (50272, 4, 0.8, 50, 1.0, "f16"), (50272, 4, 0.8, 0, 0.9, "f32"), (50272, 4, 1.0, 50, 0.9, "bf16"), (32000, 6, 1.0, 1000, 0.95, "f16"),
         (131072, 4, 0.7, 0, 0.95, "f16")]
FLAT = (50272, 2, 1.0, 0, 0.9, "f16")        # validity and the kept_n sandwich only: tokens below delta in probability are interchangeable
ROWS, COUNTERS = 16, 128
SEED = 0x1234567890ABCDEF
COUNTER0 = 1000


class Oracle:
    def __init__(self, vals, temperature=1.0, top_k=0, top_p=1.0, eps=EPS):
        vals = np.asarray(vals, dtype=np.float64)
        n = vals.shape[0]
        T, P = float(np.float32(temperature)), float(np.float32(top_p))          # the kernel reads fp32 parameters
        assert T > 0
        z = vals / T
        cand = np.nonzero(z > -np.inf)[0]
        assert cand.size and np.isfinite(z[cand]).all(), "the oracle is for ordinary rows"
        order = cand[np.argsort(-z[cand], kind="stable")]                        # z descending, ties by smaller index
        if 0 < top_k < n:
            order = order[:top_k]
        w = np.exp(z - z[order[0]])
        wo = w[order]
        zk = wo.sum()
        before = (np.cumsum(wo) - wo) / zk                                       # the summed p of the entries strictly before, in the order
        if P < 1.0:
            keep = max(1, int((before < P).sum()))
            self.n_lo = max(1, int((before < P - eps).sum()))
            self.n_hi = max(1, int((before < P + eps).sum()))
        else:
            keep = self.n_lo = self.n_hi = order.size
        self.order, self._cum_order, self.zk = order, np.cumsum(wo), zk
        self.kept_n = keep
        self.kept_mass = self.mass_of(keep) if P < 1.0 else 1.0
        self.survivors = np.sort(order[:keep])                                   # index order
        ws = w[self.survivors]
        self.C = np.cumsum(ws)
        self.Z = self.C[-1]
        self.w = w
        self.prob = np.zeros(n)
        self.prob[self.survivors] = ws / self.Z

    def mass_of(self, kept_n):
        """the top-k survivors' mass in the first kept_n entries of the order"""
        return float(self._cum_order[int(kept_n) - 1] / self.zk)

    def draw(self, u):
        """the token of the contract for uniform(s) u, in fp64"""
        i = np.minimum(np.searchsorted(self.C, np.asarray(u) * self.Z, side="right"), self.survivors.size - 1)
        return self.survivors[i]

    def bounds(self, u, delta=DELTA):
        """positions [lo, hi] (inclusive) in `survivors` of the acceptable tokens for uniform(s) u"""
        t = np.asarray(u, dtype=np.float64) * self.Z
        last = self.survivors.size - 1
        lo = np.minimum(np.searchsorted(self.C, t - delta * self.Z, side="right"), last)     # first i with C_i + delta Z > t
        hi = np.minimum(np.searchsorted(self.C, t + delta * self.Z, side="right"), last)     # last i with C_(i-1) - delta Z <= t
        return lo, hi

    def accepts(self, u, tok, delta=DELTA):
        lo, hi = self.bounds(u, delta)
        tok = np.asarray(tok)
        pos = np.minimum(np.searchsorted(self.survivors, tok), self.survivors.size - 1)
        return (self.survivors[pos] == tok) & (lo <= pos) & (pos <= hi)

    def logprob(self, tok):
        with np.errstate(divide="ignore"):
            return np.log(self.prob[np.asarray(tok)])
