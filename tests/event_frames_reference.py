"""numpy restatements the event-frame kernels (csrc/ren_event_frames.hip) are held to: the per-window count images and the
nine per-window comparison sums in float64.  No GPU, no product code."""
import math

import numpy as np

N_SUMS = 9


def count_images(position, timestamp, polarity, edges, height, width):
    """position (N, 2) integer (x, y), timestamp (N,) int64, polarity (N,) bool, edges (V + 1,) non-decreasing int64 ->
    (V, 2, H, W) int32, plane 0 positive / plane 1 negative: event e is in window v iff edges[v] <= t_e < edges[v + 1]"""
    position = np.asarray(position).astype(np.int64).reshape(-1, 2)
    ts = np.asarray(timestamp).astype(np.int64)
    pol = np.asarray(polarity).astype(bool)
    edges = np.asarray(edges).astype(np.int64)
    V = len(edges) - 1
    v = np.searchsorted(edges, ts, side="right") - 1
    x, y = position[:, 0], position[:, 1]
    keep = (v >= 0) & (v < V) & (x < width) & (y < height)
    out = np.zeros((V, 2, height, width), np.int32)
    np.add.at(out, (v[keep], np.where(pol[keep], 0, 1), y[keep], x[keep]), 1)
    return out


def count_images_loop(position, timestamp, polarity, edges, height, width):
    """the definition, literally: one Python step per event and window"""
    V = len(edges) - 1
    out = np.zeros((V, 2, height, width), np.int32)
    for (x, y), t, p in zip(np.asarray(position).tolist(), np.asarray(timestamp).tolist(), np.asarray(polarity).tolist()):
        if x >= width or y >= height:
            continue
        for v in range(V):
            if int(edges[v]) <= t < int(edges[v + 1]):
                out[v, 0 if p else 1, y, x] += 1
    return out


def compare_terms(counts, pred, valid, c_p, c_n):
    """(V, 9, H * W) float64: the term every pixel contributes to each of the nine sums (0 where valid == 0)"""
    counts = np.asarray(counts)
    V = counts.shape[0]
    ok = np.asarray(valid).reshape(V, -1) != 0
    npos, nneg = counts[:, 0].reshape(V, -1).astype(np.float64), counts[:, 1].reshape(V, -1).astype(np.float64)
    m = np.float64(c_p) * npos - np.float64(c_n) * nneg
    p = np.asarray(pred).reshape(V, -1).astype(np.float64)
    d = p - m
    terms = np.stack([np.ones_like(m), m, p, m * m, p * p, m * p, d * d,
                      (np.abs(d) <= max(float(c_p), float(c_n))).astype(np.float64),
                      ((npos + nneg) > 0).astype(np.float64)], 1)
    return np.where(ok[:, None, :], terms, 0.0)


def compare_sums(counts, pred, valid, c_p, c_n):
    """-> (sums (V, 9) float64 [count, sum m, sum p, sum m^2, sum p^2, sum m p, sum (p - m)^2, #explained, #active],
           abs_sums (V, 9): the sums of the terms' magnitudes, which scale the fp64 summation bound);
    the sums are math.fsum's: the correctly rounded sum of the float64 terms"""
    t = compare_terms(counts, pred, valid, c_p, c_n)
    sums = np.array([[math.fsum(t[v, k].tolist()) for k in range(N_SUMS)] for v in range(t.shape[0])], np.float64)
    return sums.reshape(t.shape[0], N_SUMS), np.abs(t).sum(-1)
