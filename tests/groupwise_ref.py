"""The fp64 reference of the group-wise dequant-GEMM (include/quip_amd_groupwise.h), written from its formula:

    y[b, r] = bias[r] + sum_g scale[r, g] * sum_{k in [g G, (g + 1) G)} (code[r, k] - zero[r, g]) * x[b, k]

in NumPy on the 16-bit-rounded x the kernel is given, plus the [m, d / G] -> group-major [d / G, m] transposition of the two tables.
A plain module (no fixtures): the GPU tests import it."""
import numpy as np
import torch


def group_major(table):
    """[m, d / G] (what the quantiser returns) -> contiguous float32 [d / G, m] (what the kernel reads)"""
    return np.ascontiguousarray(np.asarray(table, dtype=np.float32).T)


def dense_weight(codes, scale, zero, G):
    """the fp64 weight the layer stands for: scale[r, k // G] * (code[r, k] - zero[r, k // G]); scale, zero [m, d / G]"""
    codes = np.asarray(codes, dtype=np.float64)
    m, d = codes.shape
    s = np.repeat(np.asarray(scale, dtype=np.float64), G, axis=1)
    z = np.repeat(np.asarray(zero, dtype=np.float64), G, axis=1)
    assert s.shape == (m, d) and z.shape == (m, d)
    return s * (codes - z)


def x64(x):
    """a 16-bit torch tensor (the kernel's input, already rounded) as float64"""
    return x.detach().cpu().to(torch.float64).numpy()


def gemm(x, codes, scale, zero, G, bias=None):
    """y [bs, m] in float64, group by group as the formula is written; x: float64 [bs, d]"""
    codes = np.asarray(codes, dtype=np.float64)
    scale, zero = np.asarray(scale, dtype=np.float64), np.asarray(zero, dtype=np.float64)
    m, d = codes.shape
    y = np.zeros((x.shape[0], m), dtype=np.float64)
    for g in range(d // G):
        k = slice(g * G, (g + 1) * G)
        y += (x[:, k] @ (codes[:, k] - zero[:, g:g + 1]).T) * scale[:, g][None, :]
    if bias is not None:
        y += np.asarray(bias, dtype=np.float64)[None, :]
    return y


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))
