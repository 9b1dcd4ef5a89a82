"""Relay-BP: min-sum legs with a memory term per bit (Mueller et al., 2025, "Improved belief propagation is sufficient for
real-time decoding of quantum memory"), as a mode of :class:`bp_osd_amd.BpOsdDecoder`.

``BpOsdDecoder(..., relay=RelayConfig(...))`` (or ``set_relay``) makes the BP stage of every decode call of that decoder run
``bp_relay_kernel``; DESIGN.md §4.18 and the comment at ``bposd_set_relay`` in include/bposd_mi355x.h hold the definition.
This module holds the configuration object, a generator of memory strengths and the definition restated in numpy
(:func:`relay_decode_reference`), which is what the device results are compared with bit for bit.  The default strengths of
:func:`relay_gammas` are this project's choice of a starting point; nothing here claims that they are tuned.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

__all__ = ["RelayConfig", "relay_gammas", "relay_decode_reference", "RelayReferenceDecoder"]

_DBL_MAX = np.finfo(np.float64).max


class RelayConfig:
    """The relay mode of a decoder: ``gammas`` float64 [legs, n] (finite; negative values allowed), ``leg_iters`` int [legs]
    (each >= 1), ``stop_after`` >= 1 solutions end a shot, ``leg_init`` 0 resets the bit->check messages to the priors at the
    start of every leg after the first, 1 hands them on.  ValueError names what is wrong."""

    def __init__(self, gammas, leg_iters, stop_after=1, leg_init=0):
        g = np.array(gammas, dtype=np.float64, order="C")
        if g.ndim != 2 or g.shape[0] < 1 or g.shape[1] < 1:
            raise ValueError(f"gammas must have shape (legs, n) with legs >= 1, not {g.shape}")
        if not np.isfinite(g).all():
            r, j = np.argwhere(~np.isfinite(g))[0]
            raise ValueError(f"gammas[{r}][{j}] = {g[r, j]} is not finite")
        it = np.asarray(leg_iters)
        if it.ndim != 1 or it.shape[0] != g.shape[0] or not np.issubdtype(it.dtype, np.integer):
            raise ValueError(f"leg_iters must hold {g.shape[0]} integers (one per row of gammas), not {it.shape} {it.dtype}")
        if (it < 1).any() or (it > np.iinfo(np.int32).max).any():
            r = int(np.nonzero((it < 1) | (it > np.iinfo(np.int32).max))[0][0])
            raise ValueError(f"leg_iters[{r}] = {it[r]} must be at least 1")
        if int(stop_after) != stop_after or int(stop_after) < 1:
            raise ValueError(f"stop_after = {stop_after} must be an integer >= 1")
        if leg_init not in (0, 1):
            raise ValueError(f"leg_init = {leg_init} must be 0 (reset the messages) or 1 (keep them)")
        self.gammas = g
        self.gammas.setflags(write=False)
        self.leg_iters = np.ascontiguousarray(it, dtype=np.int32)
        self.leg_iters.setflags(write=False)
        self.stop_after = int(stop_after)
        self.leg_init = int(leg_init)

    def restrict(self, bits):
        """The same legs on a subset of the bits (``gammas[:, bits]``): what one window of a windowed decode runs with when
        the configuration is given over all faults of the model."""
        return RelayConfig(self.gammas[:, np.asarray(bits, dtype=np.int64)], self.leg_iters, self.stop_after, self.leg_init)

    @property
    def legs(self):
        return self.gammas.shape[0]

    @property
    def n(self):
        return self.gammas.shape[1]

    @property
    def total_iters(self):
        return int(self.leg_iters.sum())

    def __repr__(self):
        return (f"RelayConfig(legs={self.legs}, n={self.n}, leg_iters={self.leg_iters.tolist()}, stop_after={self.stop_after}, "
                f"leg_init={self.leg_init})")


def relay_gammas(n, legs, gamma0=0.125, gamma_range=(-0.24, 0.66), seed=0):
    """Memory strengths [legs, n]: row 0 is the constant ``gamma0``, rows >= 1 are uniform in ``gamma_range`` per bit and leg
    (``numpy.random.default_rng(seed)``).  The defaults are a starting point of this project's, not tuned values."""
    n, legs = int(n), int(legs)
    if n < 1 or legs < 1:
        raise ValueError("n and legs must be at least 1")
    lo, hi = float(gamma_range[0]), float(gamma_range[1])
    g = np.empty((legs, n), np.float64)
    g[0] = float(gamma0)
    if legs > 1:
        g[1:] = lo + (hi - lo) * np.random.default_rng(seed).random((legs - 1, n))
    return g


def _prior_llr(p):
    """log((1 - p) / p) elementwise with the platform's libm (as the library's host code forms it): +inf at 0, -inf at 1."""
    p = np.asarray(p, dtype=np.float64)
    if np.any(~((p >= 0) & (p <= 1))):
        raise ValueError("channel probabilities must lie in [0, 1]")
    with np.errstate(divide="ignore"):
        q = (1 - p) / p
    out = np.empty(q.shape, np.float64)
    flat_q, flat_o = q.reshape(-1), out.reshape(-1)
    for k in range(flat_q.size):
        x = flat_q[k]
        flat_o[k] = -math.inf if x == 0.0 else (math.inf if x == math.inf else math.log(x))
    return out


def _alpha(ms_scaling_factor, t):
    """The scaling factor of iteration t (one value per shot)."""
    if ms_scaling_factor != 0.0:
        return np.full(t.shape, float(ms_scaling_factor))
    return np.where(t > 1074, 1.0, 1.0 - np.ldexp(1.0, -np.minimum(t, 1074)))


def relay_decode_reference(H, syndromes, priors, cfg, ms_scaling_factor=1.0, prior_select=None, alt_priors=None):
    """The definition of the relay mode in numpy, vectorised over the shots.

    H : (m, n) parity-check matrix (dense or scipy.sparse); syndromes : [B, m]; priors : error probabilities [n], or [B, n]
    for a channel per shot; ``prior_select`` [B, n] with ``alt_priors`` [n] is the two-valued form (``alt_priors[j]`` where the
    selector is set).  Returns a dict of ``osdw / osd0 / bp`` (uint8 [B, n]; the three are equal: there is no OSD stage
    here), ``converged`` (bool [B]), ``iters`` (int32 [B]), ``solutions`` (int32), ``best_leg`` (int32, -1: none), ``weight``
    (int64) and ``llr`` (float64 [B, n], the final memory M)."""
    Hc = sp.csr_matrix(H).astype(np.int64)
    Hc.data %= 2
    Hc.eliminate_zeros()
    Hc.sum_duplicates()
    Hc.sort_indices()
    m, n = Hc.shape
    if cfg.n != n:
        raise ValueError(f"the relay configuration is for {cfg.n} bits, the matrix has {n}")
    rp, ci = Hc.indptr.astype(np.int64), Hc.indices.astype(np.int64)
    # edges of a column in ascending row order (= ascending CSR edge id)
    ce = np.argsort(ci, kind="stable")
    cp = np.concatenate(([0], np.cumsum(np.bincount(ci, minlength=n)))).astype(np.int64)
    cdeg, vdeg = np.diff(rp), np.diff(cp)
    # k-th edge of every check that has one, q-th edge of every bit that has one
    chk_k = [np.nonzero(cdeg > k)[0] for k in range(int(cdeg.max(initial=0)))]
    bit_q = [np.nonzero(vdeg > q)[0] for q in range(int(vdeg.max(initial=0)))]

    s = (np.asarray(syndromes).astype(np.int64) & 1).astype(bool)
    if s.ndim != 2 or s.shape[1] != m:
        raise ValueError(f"The syndromes must have shape (B, {m}). Not {s.shape}.")
    B = s.shape[0]
    p = np.asarray(priors, dtype=np.float64)
    if p.shape == (n,):
        l0 = np.broadcast_to(_prior_llr(p), (B, n))
        if prior_select is not None:
            sel = np.asarray(prior_select) != 0
            l0 = np.where(sel, _prior_llr(np.asarray(alt_priors, dtype=np.float64))[None, :], l0)
    elif p.shape == (B, n) and prior_select is None:
        l0 = _prior_llr(p)
    else:
        raise ValueError(f"priors must have shape ({n},) or ({B}, {n}), not {p.shape}")
    l0 = np.ascontiguousarray(l0)
    W = np.rint(np.clip(l0, -32768.0, 32768.0) * 4294967296.0).astype(np.int64)

    M = l0.copy()
    dec = np.zeros((B, n), np.uint8)
    best = np.zeros((B, n), np.uint8)
    msg = l0[:, ci].copy()  # [B, E] by CSR edge
    t = np.zeros(B, np.int64)
    found = np.zeros(B, np.int32)
    best_leg = np.full(B, -1, np.int32)
    best_w = np.zeros(B, np.int64)
    done = ~s.any(axis=1)  # all-zero syndrome: nothing runs

    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(cfg.legs):
            g = cfg.gammas[r]
            om = 1.0 - g
            live = ~done
            if not live.any():
                break
            if r > 0 and cfg.leg_init == 0:
                msg[live] = l0[live][:, ci]
            in_leg = live.copy()
            for _ in range(int(cfg.leg_iters[r])):
                idx = np.nonzero(in_leg)[0]
                if idx.size == 0:
                    break
                t[idx] += 1
                alpha = _alpha(ms_scaling_factor, t[idx])[:, None]
                v = msg[idx]
                neg = v <= 0.0  # a zero counts as negative
                av = np.abs(v)
                # ---- check pass: prefix and suffix minima from DBL_MAX, parity of the signs and the syndrome
                pre = np.empty_like(v)
                run = np.full((idx.size, m), _DBL_MAX)
                par = s[idx].copy()
                for k, cs in enumerate(chk_k):
                    e = rp[cs] + k
                    pre[:, e] = run[:, cs]
                    a = av[:, e]
                    run[:, cs] = np.where(a < run[:, cs], a, run[:, cs])
                    par[:, cs] ^= neg[:, e]
                c2b = np.empty_like(v)
                run = np.full((idx.size, m), _DBL_MAX)
                for k in range(len(chk_k) - 1, -1, -1):
                    cs = chk_k[k]
                    e = rp[cs] + k
                    mag = np.where(run[:, cs] < pre[:, e], run[:, cs], pre[:, e])
                    val = mag * alpha
                    c2b[:, e] = np.where(par[:, cs] ^ neg[:, e], -val, val)
                    a = av[:, e]
                    run[:, cs] = np.where(a < run[:, cs], a, run[:, cs])
                # ---- bit pass: the sums start at lam = (1 - g) * l0 + g * M
                lam = om[None, :] * l0[idx] + g[None, :] * M[idx]
                acc = lam.copy()
                b2c = np.empty_like(v)
                for q, bs in enumerate(bit_q):
                    e = ce[cp[bs] + q]
                    b2c[:, e] = acc[:, bs]
                    acc[:, bs] = acc[:, bs] + c2b[:, e]
                suf = np.zeros((idx.size, n))
                for q in range(len(bit_q) - 1, -1, -1):
                    bs = bit_q[q]
                    e = ce[cp[bs] + q]
                    b2c[:, e] = b2c[:, e] + suf[:, bs]
                    suf[:, bs] = suf[:, bs] + c2b[:, e]
                M[idx] = acc
                d = (acc <= 0.0).astype(np.uint8)
                dec[idx] = d
                msg[idx] = b2c
                # ---- H dec == syndrome ?
                cand = np.asarray((Hc @ d.T.astype(np.int64)).T)
                sol = ((cand & 1).astype(bool) == s[idx]).all(axis=1)
                hit = idx[sol]
                if hit.size:
                    w = (dec[hit].astype(np.int64) * W[hit]).sum(axis=1)
                    better = (found[hit] == 0) | (w < best_w[hit])
                    bi = hit[better]
                    best[bi] = dec[bi]
                    best_w[bi] = w[better]
                    best_leg[bi] = r
                    found[hit] += 1
                    in_leg[hit] = False
                    done[hit[found[hit] == cfg.stop_after]] = True

    has = found > 0
    bp = np.where(has[:, None], best, dec).astype(np.uint8)
    conv = has | ~s.any(axis=1)
    return {"osdw": bp.copy(), "osd0": bp.copy(), "bp": bp, "converged": conv, "iters": t.astype(np.int32), "solutions": found,
            "best_leg": best_leg, "weight": best_w, "llr": M}


class RelayReferenceDecoder:
    """:func:`relay_decode_reference` behind the decoder surface the simulation classes drive: usable as
    ``decoder_factory=RelayReferenceDecoder`` with ``relay=cfg`` among the decoder keyword arguments (``engine="numpy"``).
    It has no OSD stage: ``osd_method`` must be "osd_off" (shots without a solution keep their last BP decisions)."""

    def __init__(self, pcm, channel_probs=None, error_rate=None, relay=None, ms_scaling_factor=1.0, bp_method="minimum_sum",
                 schedule="parallel", osd_method="osd_off", **ignored):
        if not isinstance(relay, RelayConfig):
            raise ValueError("relay= must be a RelayConfig")
        if str(bp_method).lower() not in ("minimum_sum", "min_sum", "ms", "1") or str(schedule).lower() != "parallel":
            raise ValueError("relay mode needs min-sum and the flooding schedule")
        if str(osd_method).lower() not in ("osd_off", "off"):
            raise ValueError("the relay reference has no OSD stage: osd_method must be 'osd_off'")
        self._H = sp.csr_matrix(pcm)
        self.m, self.n = self._H.shape
        if relay.n != self.n:
            raise ValueError(f"the relay configuration is for {relay.n} bits, this decoder has {self.n}")
        self._probs = np.full(self.n, float(error_rate)) if channel_probs is None else np.array(channel_probs, dtype=np.float64)
        self._cfg = relay
        self._ms = float(ms_scaling_factor)
        self.last = None

    def update_channel_probs(self, channel_probs):
        self._probs = np.array(channel_probs, dtype=np.float64)

    def decode_batch(self, syndromes, prior_select=None, alt_channel_probs=None, channel_probs_rows=None, **kw):
        """The per-shot channel forms of ``BpOsdDecoder.decode_batch`` are honoured; any other option that would change the
        result is refused (the output selectors ``want_*`` are accepted: the dict always holds everything)."""
        other = sorted(k for k in kw if not k.startswith("want_"))
        if other:
            raise ValueError(f"RelayReferenceDecoder.decode_batch does not take {other}")
        if channel_probs_rows is not None and prior_select is not None:
            raise ValueError("channel_probs_rows cannot be combined with prior_select")
        if (prior_select is None) != (alt_channel_probs is None):
            raise ValueError("prior_select and alt_channel_probs go together")
        priors = self._probs if channel_probs_rows is None else np.asarray(channel_probs_rows, dtype=np.float64)
        self.last = relay_decode_reference(self._H, syndromes, priors, self._cfg, self._ms, prior_select=prior_select,
                                           alt_priors=alt_channel_probs)
        return self.last
