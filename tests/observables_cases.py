"""The observable matrices and references of tests/test_observables_cpu.py and tests/test_gpu_observables.py.

The codes, settings and syndromes are those of tests/channel_rows_cases.py (read only); the reference for an observable is
``(oracle_rows @ L.T) & 1`` in numpy on the rows of ``uniform_reference`` -- never on rows a GPU produced.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import channel_rows_cases as cr


@functools.lru_cache(maxsize=None)
def edge_matrix(n, k):
    """L [k, n] uint8: density 0.5 from default_rng(11), with the rows that pin the edges of the packed layout overwritten --
    0 empty, 1 all ones, 2 the last column only, 3 the first column only, k - 1 the first bit of the last word only."""
    L = (np.random.default_rng(11).random((k, n)) < 0.5).astype(np.uint8)
    for row, cols in ((0, []), (1, range(n)), (2, [n - 1]), (3, [0]), (k - 1, [(n - 1) & ~63])):
        if row < k:
            L[row] = 0
            L[row, list(cols)] = 1
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def plain_matrix(n, k):
    """A plain random L (seed 11, density 0.5): what the honesty figures of the issue were measured with."""
    L = (np.random.default_rng(11).random((k, n)) < 0.5).astype(np.uint8)
    L.setflags(write=False)
    return L


def observables(rows, L):
    """uint8 [B, k]: the reference product over GF(2)."""
    return ((np.asarray(rows).astype(np.int64) @ L.T.astype(np.int64)) & 1).astype(np.uint8)


def pack(bits):
    """uint8 [B, k] -> uint64 [B, ceil(k/64)], bit (j & 63) of word (j >> 6) = entry j, padding zero."""
    by = np.packbits(np.ascontiguousarray(bits, dtype=np.uint8), axis=1, bitorder="little")
    out = np.zeros((bits.shape[0], 8 * ((bits.shape[1] + 63) // 64)), np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u8")


def reference(case_id, L):
    """The oracle's decode of the case's syndromes on the constructor channel, as observables of L."""
    ref = cr.uniform_reference(case_id)
    return dict(osdw=observables(ref["osdw"], L), osd0=observables(ref["osd0"], L), bp=observables(ref["bp"], L),
                converged=np.asarray(ref["converged"]).astype(bool), iters=np.asarray(ref["iters"]))
