"""Shared helpers of the sparse-conv kernel tests (a plain module, like tests/abi_contract.py): float64 references of the three
conv passes over an (n, K) neighbour map, and a builder of synthetic maps with any row count, any K and chosen edge patterns.

A map is int32 (n, K): map[i][k] = the source row that result row i gathers at offset k, or -1.  Every column is injective (no source
row appears twice under one offset), as in a rulebook.  Only the present pairs are summed."""
import numpy as np
import torch


def f64_conv(src, W, nbr, transpose):
    """float64 reference: dst[i] = sum_k src[nbr[i][k]] @ W[k] (or W[k]^T), over the present pairs; numpy arrays in and out.
    Large maps are summed with torch float64 on the CPU (the same arithmetic, faster gathers)."""
    K = nbr.shape[1]
    W = W.reshape(K, W.shape[-2], W.shape[-1]).astype(np.float64)
    if nbr.size > (1 << 20):
        return _f64_conv_torch(torch.from_numpy(np.asarray(src, np.float64)), torch.from_numpy(W), torch.from_numpy(np.asarray(nbr)),
                               transpose).numpy()
    s64 = src.astype(np.float64)
    out = np.zeros((nbr.shape[0], W.shape[1] if transpose else W.shape[2]))
    for k in range(K):
        rows = np.nonzero(nbr[:, k] >= 0)[0]
        if rows.size:
            out[rows] += s64[nbr[rows, k]] @ (W[k].T if transpose else W[k])
    return out


def _f64_conv_torch(s64, W64, nbr, transpose):
    out = torch.zeros((nbr.shape[0], W64.shape[1] if transpose else W64.shape[2]), dtype=torch.float64)
    for k in range(nbr.shape[1]):
        col = nbr[:, k].long()
        rows = torch.nonzero(col >= 0).squeeze(1)
        if rows.numel():
            out.index_add_(0, rows, s64[col[rows]] @ (W64[k].t() if transpose else W64[k]))
    return out


def wgrad64(feat, dout, nbr_out, K, cin, cout):
    """dW[k] = sum_i feat[nbr_out[i][k]]^T dout[i] in float64 on the tensors' device"""
    f, d = feat.double(), dout.double()
    out = torch.zeros((K, cin, cout), dtype=torch.float64, device=feat.device)
    for k in range(K):
        col = nbr_out[:, k].long()
        rows = torch.nonzero(col >= 0).squeeze(1)
        if rows.numel():
            out[k] = f[col[rows]].t() @ d[rows]
    return out


def transpose_map(nbr_out, n_src):
    """the backward map of nbr_out: nbr_in[j][k] = i where nbr_out[i][k] = j (columns injective), -1 elsewhere"""
    n, K = nbr_out.shape
    nbr_in = np.full((n_src, K), -1, np.int32)
    i, k = np.nonzero(nbr_out >= 0)
    nbr_in[nbr_out[i, k], k] = i
    return nbr_in


EDGES = ("empty_rows", "full_rows", "offset_gap_tiles", "last_row_only")


def synth_map(rng, n, K, n_src=None, pairs_per_row=8.0, edges=EDGES, one_per_source=False, tile=64):
    """-> (nbr_out (n, K), nbr_in (n_src, K), order (n,)) int32: a map of exactly n result rows over n_src source rows (default n), its
    consistent transpose and a row-order hint (a permutation of the result rows).

    edges (any subset of EDGES):
      empty_rows       every 13th row has no neighbour at all
      full_rows        the last row, and the row in the middle of the second tile, gather at all K offsets
      offset_gap_tiles offset K // 2 is absent from every even-numbered `tile`-row tile
      last_row_only    offset K - 1 is present in the last row of the last (partial) tile only
    one_per_source: every source row appears in exactly one (row, offset) pair (a layer whose stride equals its kernel); n_src is
    then the number of pairs and `edges` is ignored"""
    if one_per_source:
        slots = n * K
        m = min(slots, max(1, int(round(n * min(pairs_per_row, K)))))
        pick = rng.choice(slots, size=m, replace=False)
        nbr = np.full(slots, -1, np.int32)
        nbr[pick] = rng.permutation(m).astype(np.int32)
        nbr = nbr.reshape(n, K)
        return nbr, transpose_map(nbr, m), rng.permutation(n).astype(np.int32)
    n_src = n if n_src is None else n_src
    mask = rng.random((n, K)) < min(0.9, pairs_per_row / K)
    if "offset_gap_tiles" in edges and K > 1:
        for t in range(0, (n + tile - 1) // tile, 2):
            mask[t * tile:(t + 1) * tile, K // 2] = False
    if "last_row_only" in edges and K > 1:
        mask[:, K - 1] = False
    if "empty_rows" in edges:
        mask[::13] = False
    if "full_rows" in edges and n > 0:
        mask[n - 1] = True
        if n > tile + tile // 2:
            mask[tile + tile // 2, :K - 1] = True
    if "last_row_only" in edges and n > 0:
        mask[n - 1, K - 1] = True
    nbr = np.full((n, K), -1, np.int32)
    for k in range(K):
        rows = np.nonzero(mask[:, k])[0]
        if rows.size > n_src:
            rows = np.sort(rng.choice(rows, size=n_src, replace=False))
            if mask[n - 1, k] and rows[-1] != n - 1:
                rows[-1] = n - 1
        nbr[rows, k] = rng.choice(n_src, size=rows.size, replace=False)
    return nbr, transpose_map(nbr, n_src), rng.permutation(n).astype(np.int32)

