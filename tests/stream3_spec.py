"""NumPy specification of layout 2 ("STREAM3"): 3-bit codes at exactly 3 bits per weight, in the order the fused
dequant-GEMM of csrc/dqgemm_w3.hip streams.  A helper module of the tests, not a test file.

A code c = lo + 4 * hi is split into a 2-bit low plane (lo = c & 3) and a 1-bit high plane (hi = c >> 2).  Per row tile
(16 output rows) and k-chunk (256 input columns) the low plane is BYTE FOR BYTE the 2-bit STREAM tile of `codes & 3`
(oracle.quip_oracle.pack_stream(codes & 3, 2): 64 lanes x 4 dwords = 1 KiB) and the high plane is 64 lanes x 2 dwords
= 512 B.  One row tile is stored as one contiguous run of nkc * 1536 bytes (nkc = d / 256), in blocks of 768 words (3 KiB) per
PAIR of chunks -- low tile, low tile, high bits, high bits -- so that a kernel stage of two chunks reads one contiguous block:

    word offset of row tile rt:            rt * nkc * 384
      + low tile of chunk c:               (c // 2) * 768 + (c % 2) * 256 + lane * 4 + u      (u = 0..3)
      + high bits of chunk c:              (c // 2) * 768 + 512 + (c % 2) * 128 + lane * 2 + w   (w = 0..1)
        (an unpaired last chunk, nkc odd:  (c // 2) * 768 + 256 + lane * 2 + w)

so a 16-byte-per-lane transfer of 64 lanes moves one low tile, or the high bits of the TWO chunks of a pair.
Lane 16 g + j owns row 16 rt + j and the columns 256 c + 32 t + 8 g + e (e = 0..7) of every MFMA step t = 0..7.

Low plane (the 2-bit STREAM rule): dword u = t // 2 holds steps 2u, 2u + 1; field i = 4 (t & 1) + e // 2 sits at bits
[2i, 2i + 2) of the lower 16-bit half for even e and of the upper half for odd e.

High plane: dword w = t // 4.  The kernel merges low and high plane into "nibble words" with one bit-field insert:
the fields of even i of low dword u (mask 0x3333 of each half) and of odd i (the same after >> 2), nibble k = i // 2.
The high bit of that code has to arrive at bit 4 k + 2 of the half after ONE shift of the whole high dword, the same
for all four nibbles.  With n = 2 (u & 1) + (i & 1) and the left shifts SH = (0, -1, 2, 1)[n] the bit is stored at
    bit (4 k + 2 - SH[n]) + 16 (e & 1)  of high dword w
(sixteen slots per half and high dword: every slot is used exactly once).
"""
import numpy as np

ROWS, KC = 16, 256
_SH = (0, -1, 2, 1)


def n_words(m, d):
    return m * d * 3 // 32


def _positions():
    """(t, e) -> (u, low shift, w, high bit)"""
    pos = {}
    for t in range(8):
        for e in range(8):
            u, i = t // 2, 4 * (t & 1) + e // 2
            half = 16 * (e & 1)
            n, k = 2 * (u & 1) + (i & 1), i // 2
            pos[t, e] = (u, 2 * i + half, t // 4, 4 * k + 2 - _SH[n] + half)
    return pos


def _offsets(c, nkc):
    """word offsets of chunk c's low tile and high bits inside its row tile's run"""
    base = (c // 2) * 768
    if (nkc & 1) and c == nkc - 1:
        return base, base + 256
    return base + (c % 2) * 256, base + 512 + (c % 2) * 128


def pack_stream3(codes):
    codes = np.asarray(codes)
    m, d = codes.shape
    assert m % ROWS == 0 and d % KC == 0 and codes.max(initial=0) < 8
    nrt, nkc = m // ROWS, d // KC
    c = codes.reshape(nrt, 16, nkc, 8, 4, 8).astype(np.uint32)             # [rt, j, c, t, g, e]
    low = np.zeros((nrt, nkc, 64, 4), dtype=np.uint32)
    high = np.zeros((nrt, nkc, 64, 2), dtype=np.uint32)
    for (t, e), (u, lsh, w, hbit) in _positions().items():
        v = np.transpose(c[:, :, :, t, :, e], (0, 2, 3, 1)).reshape(nrt, nkc, 64)   # lane = 16 g + j
        low[:, :, :, u] |= (v & np.uint32(3)) << np.uint32(lsh)
        high[:, :, :, w] |= (v >> np.uint32(2)) << np.uint32(hbit)
    out = np.zeros((nrt, nkc * 384), dtype=np.uint32)
    for c in range(nkc):
        lo, hi = _offsets(c, nkc)
        out[:, lo:lo + 256] = low[:, c].reshape(nrt, 256)
        out[:, hi:hi + 128] = high[:, c].reshape(nrt, 128)
    return out.reshape(-1).view(np.int32)


def unpack_stream3(words, m, d):
    nrt, nkc = m // ROWS, d // KC
    p = np.asarray(words).view(np.uint32).reshape(nrt, nkc * 384)
    low = np.stack([p[:, _offsets(c, nkc)[0]:][:, :256] for c in range(nkc)], axis=1).reshape(nrt, nkc, 64, 4)
    high = np.stack([p[:, _offsets(c, nkc)[1]:][:, :128] for c in range(nkc)], axis=1).reshape(nrt, nkc, 64, 2)
    codes = np.zeros((nrt, 16, nkc, 8, 4, 8), dtype=np.uint8)
    for (t, e), (u, lsh, w, hbit) in _positions().items():
        v = ((low[:, :, :, u] >> np.uint32(lsh)) & np.uint32(3)) | (((high[:, :, :, w] >> np.uint32(hbit)) & np.uint32(1)) << np.uint32(2))
        codes[:, :, :, t, :, e] = np.transpose(v.reshape(nrt, nkc, 4, 16), (0, 3, 1, 2))
    return codes.reshape(m, d)


def low_plane(words, m, d):
    """the low tiles of every row tile, concatenated: equals pack_stream(codes & 3, 2)"""
    nrt, nkc = m // ROWS, d // KC
    p = np.asarray(words).view(np.uint32).reshape(nrt, nkc * 384)
    return np.stack([p[:, _offsets(c, nkc)[0]:][:, :256] for c in range(nkc)], axis=1).reshape(-1).view(np.int32)
