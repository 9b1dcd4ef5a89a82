"""Monte-Carlo harness for detector error models (DEMs): the second engine next to ``css_decode_sim``.

A model is three things: a check matrix ``H`` (``M`` detectors x ``N`` fault mechanisms), an observable matrix ``L``
(``k x N``) and one prior per mechanism.  A shot samples the faults ``f`` (fault ``i`` fires with probability
``priors[i]``), forms the detector row ``H f`` and the true observables ``L f``, decodes the detector row to a correction
``c`` and succeeds when ``L c == L f``.  Nothing of it is CSS-shaped: circuit-level and phenomenological models run here,
where ``css_decode_sim`` is the code-capacity harness of the reference.

``engine="native"`` runs all of it in libbposd_mi355x.so (include/bposd_mi355x.h "Detector-error-model Monte-Carlo
engine"): one call per batch samples, multiplies, decodes straight to observables, compares and returns
five integers.  It needs no torch.  ``engine="numpy"`` is the same loop on the host around any decoder with a
``decode_batch``.  Both draw from the project's counter-based Philox stream (``sim.philox_uniforms``), indexed by (shot,
fault): they see the same shots whatever their batch sizes, and a CPU run reproduces a GPU run shot for shot.

Importance sampling (``sample_priors`` / ``sample_scale``) draws the faults from a harsher row ``q`` while
the decoder keeps ``priors`` as its channel, and weighs every shot by its likelihood ratio: logical error rates far below one
over the number of shots become measurable.  The per-shot log-weight is an integer sum (``importance_table``), so it is
bit-exact on both engines like everything else of a shot.

Fault sets of a fixed weight (``fault_weight`` / ``subset``) replace the Bernoulli row of a shot by a set of
exactly ``w`` mechanisms: every set of the stratum in turn, or uniformly drawn ones (``fault_subsets`` is the definition).
``dem_failure_spectrum`` runs the strata of weight 0, 1, ... and returns the weight up to which the decoder corrects every
fault set, and a logical error rate with a rigorous interval.

Per-fault sums over selected shots (``fault_sums`` / ``fault_stats``) reduce the fault rows of a batch to one
count and one weighted sum per mechanism where the rows are.  ``fit_sample_priors`` builds the cross-entropy fit of a
sampling row on them: a ``sample_priors`` that tilts only the faults that matter, found by the engine itself.

``phenomenological_dem`` builds ``(H, L, priors)`` of the repeated-measurement model of a code, so that the engine can be
used with no circuit simulator at hand; ``bp_osd_amd.circuit`` derives the circuit-level model of a Clifford circuit with
Pauli noise (``circuit_dem``), and INTEGRATION.md says how the three come out of a detector-error-model file.
"""
from __future__ import annotations

import json
import math

import numpy as np
import scipy.sparse as sp

from ._dem_base import HARVEST_ITEMS, DemSimBase, _gf2_csr, _pack, checked_model, create_dem, fault_sums_batch, harvest_batch
from .sim import _default_decoder_factory, _mod2_mul, philox4x32_10, philox_uniforms

__all__ = ["dem_decode_sim", "dem_failure_spectrum", "fault_subsets", "fit_sample_priors", "importance_table", "phenomenological_dem",
           "phenomenological_detector_times", "subset_table", "weight_distribution", "weight_multipliers"]

def phenomenological_dem(h, l, rounds, p_data, p_meas):
    """``(H, L, priors)`` of the phenomenological noise model of a code with checks ``h`` (m x n) and logicals ``l`` (k x n)
    measured for ``R = rounds`` noisy rounds and one perfect round:

        H = [ I_{R+1} (x) h | D (x) I_m ],  D[t, t] = D[t+1, t] = 1  ((R+1) x R)
        L = [ 1^T_{R+1} (x) l | 0 ]
        priors = [p_data] * (R+1) n  ++  [p_meas] * R m

    Column (t, i) of the first block is a flip of data bit i entering at round t, column (t, c) of the second a flipped
    outcome of check c at round t; detector (t, c) is the change of check c between rounds t - 1 and t.  ``R = 0`` is
    code capacity: ``(h, l, p_data)``.  H and L are scipy CSR (uint8), priors float64."""
    R = int(rounds)
    if R < 0:
        raise ValueError("rounds must be >= 0")
    h, l = _gf2_csr(h, "h"), _gf2_csr(l, "l")
    m, n = h.shape
    if l.shape[1] != n:
        raise ValueError(f"l must have {n} columns, not {l.shape[1]}")
    if R == 0:
        return h, l, np.full(n, float(p_data), np.float64)
    D = sp.lil_matrix((R + 1, R), dtype=np.uint8)
    for t in range(R):
        D[t, t] = D[t + 1, t] = 1
    H = sp.hstack([sp.kron(sp.identity(R + 1, dtype=np.uint8), h), sp.kron(D, sp.identity(m, dtype=np.uint8))], format="csr")
    L = sp.hstack([sp.kron(np.ones((1, R + 1), np.uint8), l), sp.csr_matrix((l.shape[0], R * m), dtype=np.uint8)], format="csr")
    priors = np.concatenate([np.full((R + 1) * n, float(p_data)), np.full(R * m, float(p_meas))]).astype(np.float64)
    return _gf2_csr(H, "H"), _gf2_csr(L, "L"), priors


def phenomenological_detector_times(m, rounds):
    """The time of every detector of ``phenomenological_dem`` for a code with ``m`` checks: detector (t, c) is row t m + c and
    has time t, for t = 0 .. rounds (what ``bp_osd_amd.window`` takes as ``detector_time``)."""
    return np.repeat(np.arange(int(rounds) + 1), int(m))


LOGW_ONE = 2 ** 32  # units of a log-weight increment per nat


def importance_table(priors, sample_priors):
    """``(incr int64 [N], c0 float)`` of drawing the faults from ``q = sample_priors`` in place of ``p = priors``: the one
    place that turns probabilities into the integers both engines sum.  The likelihood ratio of a shot with fault row f is

        w = exp(c0 + sum_{i: f_i = 1} a_i),  a_i = log(p_i / q_i) - log((1 - p_i) / (1 - q_i)),  c0 = sum_i log((1 - p_i) / (1 - q_i))

    and ``incr[i] = round(a_i * 2**32)``, so that ``w = exp(c0 + logw / 2**32)`` with the integer ``logw = f @ incr`` (the
    rounding moves w by at most 2^-33 relative per fired fault).  Terms with ``p_i == q_i`` are exactly 0, at 0 and 1 too.
    ``q_i == 0`` is allowed only where ``p_i == 0`` and ``q_i == 1`` only where ``p_i == 1``; ``|a_i| > 64`` (which takes in
    p_i = 0 or 1 against another q_i) and ``sum |incr| >= 2**62`` are refused: no shot can overflow.  Every refusal is a
    ValueError naming the fault.  Scalar ``math.log`` / ``math.log1p`` and ``math.fsum``: the same bits on every build."""
    p = np.ascontiguousarray(priors, dtype=np.float64)
    q = np.ascontiguousarray(sample_priors, dtype=np.float64)
    if p.ndim != 1 or q.shape != p.shape:
        raise ValueError(f"priors and sample_priors must be two vectors of one length, not {p.shape} and {q.shape}")
    incr = np.zeros(p.shape[0], np.int64)
    c_terms, total = [], 0
    for i, (pi, qi) in enumerate(zip(p.tolist(), q.tolist())):
        if not 0.0 <= pi <= 1.0:
            raise ValueError(f"the prior of fault {i} ({pi}) is not a probability")
        if not 0.0 <= qi <= 1.0:
            raise ValueError(f"the sampling probability of fault {i} ({qi}) is not a probability")
        if pi == qi:
            continue
        if qi == 0.0 or qi == 1.0:
            raise ValueError(f"fault {i} is sampled with probability {qi:g} but has prior {pi}: the weight of a shot would be unbounded")
        lb = math.log1p(-pi) - math.log1p(-qi) if pi < 1.0 else -math.inf  # log((1 - p) / (1 - q))
        a = (math.log(pi / qi) if pi > 0.0 else -math.inf) - lb
        if not abs(a) <= 64.0:  # (an infinite a: p_i is 0 or 1 and q_i is not)
            raise ValueError(f"the likelihood ratio of fault {i} (prior {pi}, sampled with {qi}) is beyond e^64")
        incr[i] = int(round(a * LOGW_ONE))
        total += abs(int(incr[i]))
        if total >= 2 ** 62:
            raise ValueError(f"the increments up to fault {i} sum to 2^62 or more: a shot's log-weight could overflow")
        c_terms.append(lb)
    return incr, math.fsum(c_terms)


MULTIPLIER_ONE = 2 ** 31 - 1  # the multiplier of the heaviest shot


def weight_multipliers(logw_fail):
    """uint32 [F]: the likelihood ratios of shots with integer log-weights ``logw_fail`` (int64, units of 2^-32, as
    ``last_batch("logw")`` has them) relative to the heaviest of them, as the integers the per-fault sums multiply by:
    ``rint(exp((lw - max lw) / 2**32) * (2**31 - 1))``.  The heaviest shot gets 2^31 - 1, a shot lighter than e^-22 of it 0.
    The one place that turns log-weights into multipliers: both engines sum the same integers."""
    lw = np.ascontiguousarray(logw_fail, dtype=np.int64).reshape(-1)
    if lw.size == 0:
        return np.zeros(0, np.uint32)
    rel = (lw - lw.max()).astype(np.float64) / LOGW_ONE  # (the difference is exact in int64: |lw| < 2^62)
    return np.rint(np.exp(rel) * MULTIPLIER_ONE).astype(np.uint32)


def _scaled_priors(p, beta):
    """sample_scale's row: p_i where p_i >= 0.5, else min(beta p_i, 0.5)."""
    return np.where(p >= 0.5, p, np.minimum(float(beta) * p, 0.5))


SUBSET_MODES = ("enumerate", "random")
SUBSET_MAX_WEIGHT = 64  # one lane of a wave per element of a set


def fault_subsets(seed, first_shot, B, n, w, mode):
    """int64 [B, w]: the fault sets of global shots ``first_shot .. first_shot + B - 1``, each ``w`` ascending positions in
    ``range(n)`` -- the definition the device sampler (dem_subset_kernel) is held against bit for bit.

    ``mode="enumerate"``: shot s is the set of rank s in colexicographic order (the combinatorial number system): from
    r = s, for j = w .. 1, c_j = the largest c with C(c, j) <= r and r -= C(c_j, j); the set is {c_1 < ... < c_w}.  Needs
    C(n, w) < 2^63 and ``first_shot + B <= C(n, w)``.  ``mode="random"``: Floyd's algorithm on the Philox stream.  Step
    i = 0 .. w - 1 with j = n - w + i draws from counter (s lo, s hi, i >> 1, 1) -- the fourth word 1 keeps it apart from the
    Bernoulli stream -- u = o[2 (i & 1)] | o[2 (i & 1) + 1] << 32, t = (u (j + 1)) >> 64, and takes j if t is already in the
    set, else t.  Every w-subset is equally likely up to the multiply-shift bias (j + 1) / 2^64 per step."""
    n, w, B, first_shot = int(n), int(w), int(B), int(first_shot)
    if mode not in SUBSET_MODES:
        raise ValueError(f"mode must be one of {SUBSET_MODES}, not {mode!r}")
    if not 0 <= w <= min(n, SUBSET_MAX_WEIGHT):
        raise ValueError(f"the weight {w} is outside [0, min(n = {n}, {SUBSET_MAX_WEIGHT})]")
    if B < 0 or first_shot < 0:
        raise ValueError("first_shot and B must be >= 0")
    out = np.zeros((B, w), np.int64)
    if mode == "enumerate":
        count = math.comb(n, w)
        if count >= 2 ** 63:
            raise ValueError(f"C({n}, {w}) is 2^63 or more: the sets of weight {w} cannot be enumerated by a 63-bit rank")
        if first_shot + B > count:
            raise ValueError(f"ranks {first_shot} .. {first_shot + B - 1}: there are only {count} sets of weight {w} on {n} faults")
        r = np.arange(B, dtype=np.uint64) + np.uint64(first_shot)
        for j in range(w, 0, -1):  # (a rank is below 2^63, so an entry clamped to 2^63 compares as the true one would)
            row = np.array([min(math.comb(c, j), 2 ** 63) for c in range(n + 1)], dtype=np.uint64)
            c = np.searchsorted(row, r, side="right").astype(np.int64) - 1
            r = r - row[c]
            out[:, j - 1] = c
        return out
    seed = int(seed) & (2 ** 64 - 1)
    s = (np.arange(B, dtype=np.uint64) + np.uint64(first_shot & (2 ** 64 - 1)))[:, None]
    pair = np.arange((w + 1) // 2, dtype=np.uint64)[None, :]
    o = philox4x32_10((s & np.uint64(0xFFFFFFFF), s >> np.uint64(32), pair, 1), (seed & 0xFFFFFFFF, seed >> 32))
    o = [np.broadcast_to(x, (B, pair.shape[1])) for x in o]
    chosen = np.full((B, w), -1, np.int64)
    for i in range(w):
        j = n - w + i
        lo, hi = o[2 * (i & 1)][:, i >> 1], o[2 * (i & 1) + 1][:, i >> 1]
        m = np.uint64(j + 1)  # (u m) >> 64 from the 32-bit halves of u: every product stays below 2^64 for m < 2^32
        t = ((hi * m + ((lo * m) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)
        taken = (chosen[:, :i] == t[:, None]).any(axis=1)
        chosen[:, i] = np.where(taken, j, t)
    return np.sort(chosen, axis=1)


def _checked_support(support, N):
    a = np.asarray(support)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("support must be a vector of fault indices")
    a = a.astype(np.int64)
    if a.size and (a[0] < 0 or a[-1] >= N or (np.diff(a) <= 0).any() or a.min() < 0 or a.max() >= N):
        raise ValueError(f"support must be strictly ascending fault indices in [0, {N})")
    return a


def subset_table(priors, support):
    """``(incr int64 [N], c0 float)`` of the probability of a fault set under ``priors``: for a set S of the support (and no
    fault outside S firing) ``P(S) = exp(c0 + sum_{i in S} incr[i] / 2**32)`` with ``incr[i] = round(log(p_i / (1 - p_i)) 2^32)``
    on the support (0 elsewhere) and ``c0 = sum_support log1p(-p_i)`` -- the integers both engines sum per shot.  A support
    entry with a prior outside (0, 1) is a ValueError.  Scalar ``math`` and ``fsum``, as :func:`importance_table`."""
    p = np.ascontiguousarray(priors, dtype=np.float64)
    if p.ndim != 1:
        raise ValueError("priors must be a vector")
    sup = _checked_support(support, p.shape[0])
    incr = np.zeros(p.shape[0], np.int64)
    terms = []
    for i in sup.tolist():
        pi = float(p[i])
        if not 0.0 < pi < 1.0:
            raise ValueError(f"the prior of fault {i} ({pi}) is not inside (0, 1): the fault belongs to no stratum of the support")
        incr[i] = int(round((math.log(pi) - math.log1p(-pi)) * LOGW_ONE))
        terms.append(math.log1p(-pi))
    return incr, math.fsum(terms)


def _weight_dp(priors, max_weight, support):
    """(P(|f| = w) for w = 0 .. max_weight, P(|f| > max_weight)) over the faults of the support, each firing independently."""
    p = np.ascontiguousarray(priors, dtype=np.float64)
    if p.ndim != 1 or ((p < 0) | (p > 1) | np.isnan(p)).any():
        raise ValueError("priors must be a vector of probabilities")
    if support is not None:
        p = p[_checked_support(support, p.shape[0])]
    W = int(max_weight)
    if W < 0:
        raise ValueError("max_weight must be >= 0")
    dist = np.zeros(W + 1, np.float64)
    dist[0], tail = 1.0, 0.0
    for pi in p.tolist():  # one more fault: a set keeps its weight or gains one
        tail += dist[W] * pi
        dist[1:] = dist[1:] * (1.0 - pi) + dist[:-1] * pi
        dist[0] *= 1.0 - pi
    return dist, tail


def weight_distribution(priors, max_weight, support=None):
    """float64 [max_weight + 1]: ``P(|f| = w)`` for w = 0 .. max_weight of the faults of ``support`` (default all) firing
    independently with ``priors``: ``prod (1 - p_i)`` times the elementary symmetric polynomial ``e_w`` of the odds
    ``p_i / (1 - p_i)``, by the recurrence over the faults -- O(n max_weight), every term non-negative (kept in probabilities,
    so that a prior of 0 or 1 needs no special case)."""
    return _weight_dp(priors, max_weight, support)[0]


class dem_decode_sim(DemSimBase):
    """See the module docstring.

    H, L, priors : the model (scipy sparse or dense 0/1 matrices of shapes (M, N) and (k, N); N floats in [0, 1])
    batch_size : shots per batch (default 4096)
    engine : "native" (everything in the library; builds ``BpOsdDecoder(H, channel_probs=priors, **decoder_kwargs)``) or
        "numpy" (host loop around ``decoder_factory(H, channel_probs=priors, **decoder_kwargs).decode_batch``)
    seed : key of the Philox stream (used as given: 0 is a seed like any other)
    target_runs : shots to run
    decoder_factory : engine="numpy" only; default the MI355X ``BpOsdDecoder``.  ``decode_batch(detectors)`` returns either a
        mapping with "osdw", "osd0", "bp", "converged", "iters", or the osdw rows with the rest left as ``batch_osd0``,
        ``batch_bp``, ``batch_converge``, ``batch_iter``
    run_sim : run at once (default) or wait for :meth:`run_decode_sim`
    sample_priors, sample_scale : importance sampling, at most one of the two.  ``sample_priors`` = q, N floats in [0, 1] the
        faults are drawn against (``u(s, i) < q_i``: the same stream and counter) while the decoder keeps ``priors``;
        ``sample_scale`` = beta >= 1 is ``q_i = p_i`` where ``p_i >= 0.5``, else ``min(beta * p_i, 0.5)``.  See below
    fault_weight, subset, support : fault sets of a fixed weight in place of Bernoulli rows (both or neither of the first two;
        they exclude ``sample_priors`` / ``sample_scale``).  A shot is a set of exactly ``fault_weight`` = w of the n faults of
        ``support`` (ascending indices; default the faults with 0 < p < 1; a fault with p = 1 belongs to no stratum and is a
        ValueError): ``subset="enumerate"`` runs the sets in colexicographic order, shot s being rank s -- ``target_runs``
        then defaults to C(n, w) and may not exceed it -- and ``subset="random"`` draws them uniformly (:func:`fault_subsets`
        defines both).  See below
    harvest : K, an int >= 0 (default 0: off).  With K > 0 the failing shots are harvested: a shot whose osdw
        observables are wrong leaves the residual ``faults ^ osdw correction``, an undetected logical fault set.  Results:
        ``min_logical_weight`` (the least residual weight of the run, an upper bound of the model's fault distance; None if
        nothing failed), ``min_logical_shot`` (its global shot; the earliest of a tie), ``min_logical_fault`` (uint8 [N]),
        ``failure_weight_counts`` (int64 [N + 1]: every failing shot by residual weight) and ``failures``: the first K
        failing shots of the run in shot order, a dict of "shot" (uint64), "weight" (int32), "residual" and "faults" (packed
        rows) and, with importance sampling, "logw" (int64).  engine="native" compacts the failing rows on the device: no batch-sized array
        crosses to the host for it
    fault_stats : True (needs ``harvest >= 1``) accumulates over the run ``fault_counts`` (int64 [N]: how often every fault
        fired) and ``failure_fault_counts`` (int64 [N]: how often it fired in a shot whose osdw observables are wrong) -- which
        mechanisms the failures are made of.  Both are unweighted counts of the shots as sampled and do not depend on the
        batch size; :meth:`output_dict` does not list them.  See :meth:`fault_sums`

    Results: ``run_count``, ``bp_converge_count``, ``bp_success_count`` (converged and observables right),
    ``osd0_success_count``, ``osdw_success_count``, ``trivial_count`` (no detector fired), ``*_logical_error_rate`` with
    ``*_logical_error_rate_eb = sqrt(L (1 - L) / runs)`` as css_decode_sim has them, ``osdw_observable_error_rates``
    (float [k]), :meth:`output_dict` and :meth:`last_batch`.

    With importance sampling every shot has the weight ``w = exp(c0 + logw / 2**32)`` of :func:`importance_table`, and the
    rates become ``*_logical_error_rate = sum(w fail) / n`` with ``*_logical_error_rate_eb = sqrt(max(sum(w^2 fail) / n -
    rate^2, 0) / n)`` (fail of bp: not converged or observables wrong).  ``weight_mean = sum(w) / n`` has expectation 1 and
    ``effective_sample_fraction = sum(w)^2 / (n sum(w^2))`` says how many plain shots the weighted ones are worth; both and
    ``sample_scale`` appear in :meth:`output_dict` only then.  The ``*_count`` attributes stay unweighted counts of the shots
    as sampled, and ``osdw_observable_error_rates`` stays unweighted too (failures per sampled shot, not a rate under
    ``priors``).  ``last_batch("logw")`` is the int64 log-weight of every shot of the last batch.

    With fault sets of a fixed weight the counts and ``*_logical_error_rate`` keep their meaning: the unweighted fraction of
    the sets that were run.  New are ``stratum_size`` = C(n, w) (a Python int), ``stratum_mass`` = P(|f| = w) under ``priors``
    (:func:`weight_distribution`) and ``{bp,osd0,osdw}_failure_mass = C(n, w) / runs * sum_fail exp(c0 + logw / 2**32)``
    with the table of :func:`subset_table` -- the estimate of P(|f| = w and the decoder fails), whose sum over w is the
    logical error rate -- and ``*_failure_mass_eb = sqrt(max(C(n, w)^2 sum_fail P^2 / runs - mass^2, 0) / runs)``, exactly 0.0
    once the whole stratum was enumerated.  ``last_batch("logw")`` is the log-probability of every set in units of 2^-32,
    less c0.  :func:`dem_failure_spectrum` runs the strata one after the other."""

    _COUNTS = ("bp_converge_count", "bp_success_count", "osd0_success_count", "osdw_success_count", "trivial_count")
    _RATES = ("bp", "osd0", "osdw")

    def __init__(self, H, L, priors, batch_size=4096, engine="native", seed=0, target_runs=None, decoder_factory=None, run_sim=True,
                 sample_priors=None, sample_scale=None, harvest=0, fault_weight=None, subset=None, support=None, fault_stats=False,
                 **decoder_kwargs):
        self._check_engine(engine, decoder_factory, "decoder")
        self._H, self._L, self._priors = checked_model(H, L, priors)
        self.M, self.N = self._H.shape
        self.K = self._L.shape[0]
        if (fault_weight is None) != (subset is None):
            raise ValueError("fault_weight and subset go together: give both, or neither to sample Bernoulli rows")
        if subset is None and support is not None:
            raise ValueError("support belongs to fault sets of a fixed weight (fault_weight and subset)")
        if subset is not None and (sample_priors is not None or sample_scale is not None):
            raise ValueError("fault sets of a fixed weight exclude sample_priors / sample_scale")
        self._init_harvest(harvest, with_logw=sample_priors is not None or sample_scale is not None or subset is not None)
        self.fault_stats = bool(fault_stats)
        if self.fault_stats and not self.harvest:
            raise ValueError("fault_stats=True needs harvest >= 1: the failing shots are the ones the harvest lists")
        p = self._priors
        self._subset = self.fault_weight = None
        self._shot0 = 0  # global shot of the run's first
        if subset is not None:
            if support is None:
                if (p == 1.0).any():
                    raise ValueError(f"the prior of fault {int(np.flatnonzero(p == 1.0)[0])} is 1: it belongs to no stratum of a fixed weight")
                support = np.flatnonzero((p > 0.0) & (p < 1.0))
            self._support = _checked_support(support, self.N)
            self._subset_incr, self._subset_c0 = subset_table(p, self._support)
            target_runs = self._init_stratum(fault_weight, subset, target_runs)
        elif target_runs is None:
            target_runs = 100
        if sample_priors is not None and sample_scale is not None:
            raise ValueError("give sample_priors or sample_scale, not both")
        self.sample_scale = None
        if sample_scale is not None:
            self.sample_scale = float(sample_scale)
            if not 1.0 <= self.sample_scale < math.inf:
                raise ValueError(f"sample_scale must be a finite number >= 1, not {sample_scale}")
            sample_priors = _scaled_priors(p, self.sample_scale)
        self._tilted = sample_priors is not None
        if self._tilted:
            q = np.ascontiguousarray(sample_priors, dtype=np.float64)
            if q.shape != (self.N,):
                raise ValueError(f"sample_priors must have length {self.N}, not {q.shape}")
            self._incr, self._c0 = importance_table(p, q)
            self._sample_priors = q
            self._reset_weighted_sums()
        self._init_run(batch_size, seed, target_runs)
        self._reset_fault_stats()
        if self._subset:
            self._reset_stratum_sums()
        self._dem = None
        if engine == "native":
            from .decoder import BpOsdDecoder

            self.decoder = BpOsdDecoder(self._H, channel_probs=p, **decoder_kwargs)
            self._native_setup()
        else:
            self.decoder = (decoder_factory or _default_decoder_factory)(self._H, channel_probs=p, **decoder_kwargs)
        if run_sim:
            self.run_decode_sim()

    # ------------------------------------------------------------------ the library's engine
    def _native_setup(self):
        from . import _lib

        lib = self._lib = _lib.load()
        dem = self._dem = create_dem(lib, self.decoder.device, self.seed, self._batch_size, self._H, self._L, self._priors, self.decoder._h)
        self.decoder._observables_installed(self.K)  # bposd_dem_create has set the decoder's table
        if self._tilted:
            _lib.check_dem(lib, dem, lib.bposd_dem_set_sampling(dem, self._sample_priors.ctypes.data, self._incr.ctypes.data))
        if self._subset:
            self._native_set_subset()

    def _native_set_subset(self):
        from . import _lib

        sup = np.ascontiguousarray(self._support, dtype=np.int32)
        rc = self._lib.bposd_dem_set_subset(self._dem, _lib.DEM_SUBSET[self._subset], self.fault_weight, sup.ctypes.data, sup.size,
                                            self._subset_incr.ctypes.data)
        _lib.check_dem(self._lib, self._dem, rc)

    def _run_batch_native(self, B):
        import ctypes as C

        from . import _lib

        c = (C.c_int64 * 5)()
        first, ask = self._shot0 + self.run_count, None
        if self.harvest:
            ask = self._harvest_ask()
            self._set_native_harvest(self._dem, "bposd_dem_set_harvest", _lib.check_dem, ask)
        _lib.check_dem(self._lib, self._dem, self._lib.bposd_dem_run(self._dem, int(first), int(B), c))
        self._last_B = B
        self._accumulate(B, [int(v) for v in c], self.last_batch("obs_fail"))
        logw = self.last_batch("logw") if self._tilted or self._subset else None
        if self._tilted:
            self._accumulate_weighted(self.last_batch("flags"), self.last_batch("converged"), logw)
        if self._subset:
            self._accumulate_stratum(self.last_batch("flags"), self.last_batch("converged"), logw)
        if self.harvest:
            info = self._native_harvest_triple(self._dem, "bposd_dem_harvest_info", _lib.check_dem)
            self._accumulate_harvest(first, info, ask, logw)
        if self.fault_stats:
            self._accumulate_fault_stats()

    def device_bytes(self):
        """engine="native": bytes of device memory the engine holds for its batches (the decoder's workspaces are its own)."""
        return self._device_bytes(self._dem, "bposd_dem_device_bytes")

    def kernel_ms(self):
        """engine="native": (dem_sample_kernel, dem_score_kernel) durations of the last batch in ms (HIP events)."""
        from . import _lib

        return self._kernel_ms(self._dem, "bposd_debug_dem_timing", _lib.check_dem)

    def __del__(self):
        dem, self._dem = getattr(self, "_dem", None), None
        if dem is not None:  # before the decoder it points to goes
            self._lib.bposd_dem_destroy(dem)

    # ------------------------------------------------------------------ the host loop
    def _run_batch_numpy(self, B):
        first = self._shot0 + self.run_count
        if self._subset:
            pos = fault_subsets(self.seed, first, B, self._support.size, self.fault_weight, self._subset)
            faults = np.zeros((B, self.N), np.uint8)
            faults[np.arange(B)[:, None], self._support[pos]] = 1
        else:
            drawn = self._sample_priors if self._tilted else self._priors
            faults = (philox_uniforms(self.seed, first, B, self.N) < drawn).astype(np.uint8)
        detectors = _mod2_mul(self._H, faults)
        truth = _mod2_mul(self._L, faults)
        r = self.decoder.decode_batch(detectors)
        if isinstance(r, dict):
            rows = {"osdw": r["osdw"], "osd0": r["osd0"], "bp": r["bp"]}
            conv, iters = np.asarray(r["converged"]), np.asarray(r["iters"])
        else:
            d = self.decoder
            rows = {"osdw": r, "osd0": d.batch_osd0, "bp": d.batch_bp}
            conv, iters = np.asarray(d.batch_converge), np.asarray(d.batch_iter)
        conv = conv.astype(bool)
        obs = {key: _mod2_mul(self._L, np.asarray(v, dtype=np.uint8) & 1) for key, v in rows.items()}
        wrong = {key: (v != truth).any(axis=1) for key, v in obs.items()}
        quiet = ~detectors.any(axis=1)
        flags = (wrong["bp"].astype(np.uint8) | (wrong["osd0"].astype(np.uint8) << 1) | (wrong["osdw"].astype(np.uint8) << 2)
                 | (quiet.astype(np.uint8) << 3))
        obs_fail = (obs["osdw"] != truth).sum(axis=0).astype(np.int32)
        self._last = {"faults": _pack(faults), "detectors": _pack(detectors), "observables": _pack(truth), "obs_bp": _pack(obs["bp"]),
                      "obs_osd0": _pack(obs["osd0"]), "obs_osdw": _pack(obs["osdw"]), "flags": flags, "converged": conv.astype(np.uint8),
                      "iters": iters.astype(np.int32), "obs_fail": obs_fail}
        counters = [int(conv.sum()), int((conv & ~wrong["bp"]).sum()), int((~wrong["osd0"]).sum()), int((~wrong["osdw"]).sum()),
                    int(quiet.sum())]
        self._accumulate(B, counters, obs_fail)
        if self._tilted:
            self._last["logw"] = faults.astype(np.int64) @ self._incr
            self._accumulate_weighted(flags, self._last["converged"], self._last["logw"])
        if self._subset:
            self._last["logw"] = faults.astype(np.int64) @ self._subset_incr
            self._accumulate_stratum(flags, self._last["converged"], self._last["logw"])
        if self.harvest:  # the osdw failures, against the osdw rows
            ask = self._harvest_ask()
            h = harvest_batch(faults, rows["osdw"], wrong["osdw"], ask)
            self._last.update({item: h[item] for item in HARVEST_ITEMS})
            self._accumulate_harvest(first, (h["fail_count"], h["min_weight"], h["min_row"]), ask, self._last.get("logw"))
        if self.fault_stats:
            self._accumulate_fault_stats()

    # ------------------------------------------------------------------ common
    def _accumulate_weighted(self, flags, converged, logw):
        """The weighted sums of one batch (after ``_accumulate``, whose plain rates it replaces) from the batch's per-shot flags,
        convergence and integer log-weights: the same arithmetic on either engine."""
        w = np.exp(self._c0 + np.asarray(logw, dtype=np.int64) / LOGW_ONE)
        w2 = w * w
        flags = np.asarray(flags)
        fail = {"bp": ((flags & 1) != 0) | (np.asarray(converged) == 0), "osd0": (flags & 2) != 0, "osdw": (flags & 4) != 0}
        S = self._wsum
        S["w"] += float(w.sum())
        S["w2"] += float(w2.sum())
        n = self.run_count
        for key, f in fail.items():
            S[key] += float(w[f].sum())
            S[key + "2"] += float(w2[f].sum())
            rate = S[key] / n
            setattr(self, f"{key}_logical_error_rate", rate)
            setattr(self, f"{key}_logical_error_rate_eb", math.sqrt(max(S[key + "2"] / n - rate * rate, 0.0) / n))
        self.weight_mean = S["w"] / n
        self.effective_sample_fraction = S["w"] * S["w"] / (n * S["w2"])

    def _reset_weighted_sums(self):
        self._wsum = dict.fromkeys(("w", "w2", "bp", "bp2", "osd0", "osd02", "osdw", "osdw2"), 0.0)
        self.weight_mean = self.effective_sample_fraction = 0.0

    def set_sampling(self, sample_priors, nominal=None, target_runs=None, first_shot=0):
        """Another sampling row on the same model, decoder and engine -- the tilted sibling of :meth:`set_fault_weight`: the
        faults are drawn against ``sample_priors`` = q from now on and every shot is weighed by its likelihood ratio under
        ``nominal`` (default ``priors``; a harsher nominal row is a level of :func:`fit_sample_priors`), through
        ``importance_table(nominal, q)``.  The decoder keeps ``priors`` as its channel.  The run starts over at global shot
        ``first_shot`` with its counters, weighted sums, harvest and fault statistics reset (``target_runs`` None: as many
        shots as before); :meth:`run_decode_sim` runs it.  Refused on a sim of fault sets of a fixed weight."""
        if self._subset:
            raise ValueError("set_sampling excludes fault sets of a fixed weight (fault_weight and subset)")
        first_shot = int(first_shot)
        if first_shot < 0:
            raise ValueError("first_shot must be >= 0")
        q = np.array(sample_priors, dtype=np.float64)
        if q.shape != (self.N,):
            raise ValueError(f"sample_priors must have length {self.N}, not {q.shape}")
        nom = self._priors if nominal is None else np.ascontiguousarray(nominal, dtype=np.float64)
        if nom.shape != (self.N,):
            raise ValueError(f"nominal must have length {self.N}, not {nom.shape}")
        incr, c0 = importance_table(nom, q)  # (everything is validated before anything changes)
        if self._dem is not None:
            from . import _lib

            _lib.check_dem(self._lib, self._dem, self._lib.bposd_dem_set_sampling(self._dem, q.ctypes.data, incr.ctypes.data))
        self._tilted, self.sample_scale = True, None
        self._sample_priors, self._incr, self._c0 = q, incr, c0
        self._shot0 = first_shot
        self._reset_weighted_sums()
        self._init_harvest(self.harvest, with_logw=True)
        self._init_run(self._batch_size, self.seed, self.target_runs if target_runs is None else target_runs)
        self._reset_fault_stats()

    # ------------------------------------------------------------------ per-fault sums over selected shots
    def fault_sums(self, select="failing", multipliers=None):
        """``(counts, sums)`` of the last batch, uint64 [N] each: in how many of the selected shots every fault fired, and
        the sum of those shots' ``multipliers`` (None without multipliers).  ``select="failing"``: the shots whose osdw
        observables are wrong, as the harvest lists them (needs ``harvest=K > 0``); ``multipliers`` is uint32 [F], aligned
        with ``last_batch("fail_rows")``.  ``select="all"``: every shot, ``multipliers`` [B].  engine="native" forms the
        sums where the rows are (fault_sums_kernel): N numbers come down in place of the rows; engine="numpy" applies the
        definition (``_dem_base.fault_sums_batch``) to ``last_batch("faults")``.  Bit-exact on both."""
        from . import _lib

        if select not in _lib.DEM_SELECT:
            raise ValueError(f"select must be one of {sorted(_lib.DEM_SELECT)}, not {select!r}")
        if select == "failing" and not self.harvest:
            raise ValueError("fault_sums('failing') needs harvest=K > 0")
        mult = None
        if multipliers is not None:
            mult = np.asarray(multipliers)
            if mult.ndim != 1 or (mult.size and (not np.issubdtype(mult.dtype, np.integer) or mult.min() < 0 or mult.max() >= 2 ** 32)):
                raise ValueError("multipliers must be a vector of integers in [0, 2^32)")
            mult = np.ascontiguousarray(mult, dtype=np.uint32)
        if self._engine == "numpy":
            words = self.last_batch("faults")
            rows = self.last_batch("fail_rows") if select == "failing" else np.arange(words.shape[0], dtype=np.int32)
            if mult is not None and mult.size != rows.size:
                raise ValueError(f"{mult.size} multipliers, but the last batch has {rows.size} {'failing ' if select == 'failing' else ''}shots")
            return fault_sums_batch(words, rows, mult, self.N)
        if not self._last_B:
            raise RuntimeError("fault_sums needs a batch that has run")
        counts = np.zeros(self.N, np.uint64)
        sums = None if mult is None else np.zeros(self.N, np.uint64)
        rc = self._lib.bposd_dem_fault_sums(self._dem, _lib.DEM_SELECT[select], None if mult is None else mult.ctypes.data,
                                            0 if mult is None else mult.size, counts.ctypes.data, None if sums is None else sums.ctypes.data)
        _lib.check_dem(self._lib, self._dem, rc)
        return counts, sums

    def fault_sums_ms(self):
        """engine="native": duration of the last fault_sums_kernel launch in ms (HIP events)."""
        import ctypes as C

        from . import _lib

        if self._dem is None:
            raise RuntimeError("fault_sums_ms needs engine='native'")
        ms = C.c_double()
        _lib.check_dem(self._lib, self._dem, self._lib.bposd_debug_dem_fault_sums_timing(self._dem, C.byref(ms)))
        return ms.value

    def _reset_fault_stats(self):
        """``fault_stats=True``: how often every fault fired in the run, and how often in a failing shot (None while off)."""
        self.fault_counts = self.failure_fault_counts = None
        if self.fault_stats:
            self.fault_counts = np.zeros(self.N, np.int64)
            self.failure_fault_counts = np.zeros(self.N, np.int64)

    def _accumulate_fault_stats(self):
        self.fault_counts += self.fault_sums("all")[0].astype(np.int64)
        self.failure_fault_counts += self.fault_sums("failing")[0].astype(np.int64)

    # ------------------------------------------------------------------ fault sets of a fixed weight
    def _init_stratum(self, fault_weight, subset, target_runs):
        """Checks the stratum (w, mode) against the support; sets its results and returns the run's ``target_runs``."""
        n = self._support.size
        if subset not in SUBSET_MODES:
            raise ValueError(f"subset must be one of {SUBSET_MODES}, not {subset!r}")
        if isinstance(fault_weight, bool) or not isinstance(fault_weight, (int, np.integer)) or not 0 <= fault_weight <= min(n, SUBSET_MAX_WEIGHT):
            raise ValueError(f"fault_weight must be an int in [0, min(n = {n}, {SUBSET_MAX_WEIGHT})], not {fault_weight!r}")
        w = int(fault_weight)
        size = math.comb(n, w)
        if subset == "enumerate":
            if size >= 2 ** 63:
                raise ValueError(f"C({n}, {w}) is 2^63 or more: the sets of weight {w} cannot be enumerated by a 63-bit rank")
            if target_runs is None:
                target_runs = size
            if self._shot0 + int(target_runs) > size:
                raise ValueError(f"target_runs = {target_runs}: there are only {size} sets of weight {w} on {n} faults")
        elif target_runs is None:
            target_runs = 100
        self._subset, self.fault_weight = subset, w
        self.stratum_size = size
        self.stratum_mass = float(weight_distribution(self._priors, w, self._support)[w])
        return target_runs

    def _reset_stratum_sums(self):
        self._ssum = dict.fromkeys(("bp", "bp2", "osd0", "osd02", "osdw", "osdw2"), 0.0)
        for key in self._RATES:
            setattr(self, f"{key}_failure_mass", 0.0)
            setattr(self, f"{key}_failure_mass_eb", 0.0)

    def set_fault_weight(self, fault_weight, subset, target_runs=None, first_shot=0):
        """Another stratum on the same model, decoder and engine (a sim made with ``fault_weight`` / ``subset`` only): the run
        starts over at global shot ``first_shot`` with its counters, sums and harvest reset; :meth:`run_decode_sim` runs it."""
        if not self._subset:
            raise ValueError("set_fault_weight needs a sim made with fault_weight and subset")
        first_shot = int(first_shot)
        if first_shot < 0:
            raise ValueError("first_shot must be >= 0")
        keep, self._shot0 = self._shot0, first_shot
        try:
            target_runs = self._init_stratum(fault_weight, subset, target_runs)
        except ValueError:
            self._shot0 = keep
            raise
        self._init_harvest(self.harvest, with_logw=True)
        self._init_run(self._batch_size, self.seed, target_runs)
        self._reset_stratum_sums()
        self._reset_fault_stats()
        if self._dem is not None:
            self._native_set_subset()

    def _accumulate_stratum(self, flags, converged, logw):
        """The failure masses of the run so far (after ``_accumulate``) from one more batch's flags, convergence and integer
        log-probabilities: the same arithmetic on either engine."""
        pr = np.exp(self._subset_c0 + np.asarray(logw, dtype=np.int64) / LOGW_ONE)  # P(set) under the priors
        flags = np.asarray(flags)
        fail = {"bp": ((flags & 1) != 0) | (np.asarray(converged) == 0), "osd0": (flags & 2) != 0, "osdw": (flags & 4) != 0}
        S, n, C = self._ssum, self.run_count, self.stratum_size
        whole = self._subset == "enumerate" and n == C
        for key, f in fail.items():
            S[key] += float(pr[f].sum())
            S[key + "2"] += float((pr[f] * pr[f]).sum())
            mass = (C / n) * S[key]
            setattr(self, f"{key}_failure_mass", mass)
            setattr(self, f"{key}_failure_mass_eb", 0.0 if whole else math.sqrt(max((C / n) * C * S[key + "2"] - mass * mass, 0.0) / n))

    def last_batch(self, what):
        """One array of the last batch: "faults", "detectors", "observables" (the true ones), "obs_bp", "obs_osd0", "obs_osdw"
        (bit-packed rows, uint64 [B, ceil(./64)]: ``BpOsdDecoder.unpack_rows`` expands them), "flags" (uint8 [B]: bit 0 bp
        wrong, 1 osd0 wrong, 2 osdw wrong, 3 no detector fired), "converged" (uint8 [B]), "iters" (int32 [B]) or "obs_fail"
        (int32 [k]: osdw failures per observable in that batch), and with importance sampling "logw" (int64 [B]: the shot's
        log-weight in units of 2^-32).  With ``harvest=K`` also "fail_rows", "fail_weight" (int32, one per failing shot of the
        batch, rows ascending), "fail_residual", "fail_faults" (packed rows of the first failing shots, as many as the run still
        missed of its K, at least one) and "min_residual" (one packed row).  engine="native" copies it from the device."""
        from . import _lib

        if what not in _lib.DEM_ITEMS:
            raise ValueError(f"what must be one of {sorted(_lib.DEM_ITEMS)}")
        if what == "logw" and not self._tilted and not self._subset:
            raise ValueError("last_batch('logw') needs importance sampling (sample_priors or sample_scale) or fault sets of a fixed weight")
        self._check_harvest_item(what)
        return self._last_batch(what, lambda: self._fetch(_lib.DEM_ITEMS, self._dem, self._lib.bposd_dem_fetch, _lib.check_dem, what))

    def output_dict(self):
        """The counters and rates as a JSON string (as css_decode_sim.output_dict returns one)."""
        out = self._results()
        if self._tilted:
            out["sample_scale"] = self.sample_scale
            out["weight_mean"] = float(self.weight_mean)
            out["effective_sample_fraction"] = float(self.effective_sample_fraction)
        if self._subset:
            out.update(fault_weight=self.fault_weight, subset=self._subset, stratum_size=self.stratum_size, stratum_mass=self.stratum_mass)
            for key in self._RATES:
                out[f"{key}_failure_mass"] = float(getattr(self, f"{key}_failure_mass"))
                out[f"{key}_failure_mass_eb"] = float(getattr(self, f"{key}_failure_mass_eb"))
        if self.harvest:
            out["min_logical_weight"] = self.min_logical_weight
        return json.dumps(out, sort_keys=True, indent=4)


def dem_failure_spectrum(H, L, priors, max_weight, shots_per_weight, batch_size=4096, engine="native", seed=0, support=None,
                         decoder_factory=None, harvest=0, **decoder_kwargs):
    """The decoder's failures by fault weight: the strata w = 0 .. ``max_weight`` of fault sets of exactly w of the n faults of
    ``support`` (default: those with 0 < p < 1), one :class:`dem_decode_sim` run each on one decoder.  A stratum with
    C(n, w) <= ``shots_per_weight`` is enumerated whole -- no statistical error -- and a larger one is estimated from
    ``shots_per_weight`` uniformly drawn sets (stratum w draws from global shot ``w << 40`` on, so that the strata do not share
    draws).  Returns a dict:

    ``strata`` : per weight a dict of ``weight``, ``mode`` ("enumerate" / "random"), ``stratum_size``, ``stratum_mass``,
        ``runs``, ``{bp,osd0,osdw}_failures`` (failing sets among those run) and ``{bp,osd0,osdw}_failure_mass`` with ``_eb``;
        with ``harvest=K`` also ``failures`` (the first K failing sets, as ``dem_decode_sim.failures``) and ``min_logical_weight``
    ``logical_error_rate_lower`` (+ ``_eb``, the drawn strata's error bars in quadrature) : the sum of the osdw failure masses
    ``tail_mass`` : P(|f| > max_weight).  The osdw logical error rate lies in [lower, lower + tail_mass], up to the error bars
        of the drawn strata
    ``corrected_weight`` : the largest t such that every stratum <= t was enumerated whole and none of its sets failed under
        osdw -- "the decoder, with these settings, corrects every fault set up to weight t", proved; -1 if weight 0 fails
    ``min_failing_weight`` : the least weight at which a set that was run failed under osdw (None if none did)"""
    shots = int(shots_per_weight)
    if shots < 1:
        raise ValueError("shots_per_weight must be >= 1")
    max_weight = int(max_weight)
    sim = dem_decode_sim(H, L, priors, batch_size=batch_size, engine=engine, seed=seed, decoder_factory=decoder_factory, run_sim=False,
                         harvest=harvest, fault_weight=0, subset="enumerate", support=support, **decoder_kwargs)
    n = sim._support.size
    if not 0 <= max_weight <= min(n, SUBSET_MAX_WEIGHT):
        raise ValueError(f"max_weight must be in [0, min(n = {n}, {SUBSET_MAX_WEIGHT})], not {max_weight}")
    strata, proved, corrected, first_fail = [], True, -1, None
    for w in range(max_weight + 1):
        whole = math.comb(n, w) <= shots
        if whole:
            sim.set_fault_weight(w, "enumerate")
        else:
            sim.set_fault_weight(w, "random", target_runs=shots, first_shot=w << 40)
        sim.run_decode_sim()
        runs = sim.run_count
        row = {"weight": w, "mode": "enumerate" if whole else "random", "stratum_size": sim.stratum_size, "stratum_mass": sim.stratum_mass,
               "runs": runs, "bp_failures": runs - sim.bp_success_count, "osd0_failures": runs - sim.osd0_success_count,
               "osdw_failures": runs - sim.osdw_success_count}
        for key in sim._RATES:
            row[f"{key}_failure_mass"] = getattr(sim, f"{key}_failure_mass")
            row[f"{key}_failure_mass_eb"] = getattr(sim, f"{key}_failure_mass_eb")
        if sim.harvest:
            row["failures"] = sim.failures
            row["min_logical_weight"] = sim.min_logical_weight
        strata.append(row)
        if row["osdw_failures"] and first_fail is None:
            first_fail = w
        proved = proved and whole and not row["osdw_failures"]
        if proved:
            corrected = w
    return {"strata": strata, "logical_error_rate_lower": math.fsum(r["osdw_failure_mass"] for r in strata),
            "logical_error_rate_lower_eb": math.sqrt(math.fsum(r["osdw_failure_mass_eb"] ** 2 for r in strata)),
            "tail_mass": float(_weight_dp(sim._priors, max_weight, sim._support)[1]), "corrected_weight": corrected,
            "min_failing_weight": first_fail}


def fit_sample_priors(H, L, priors, levels=(8.0, 1.0, 1.0), shots_per_level=4096, batch_size=4096, engine="native", seed=0, smoothing=1.0,
                      min_failures=32, **decoder_kwargs):
    """``(q, report)``: a ``sample_priors`` row for :class:`dem_decode_sim` fitted by the cross-entropy method -- the row
    that tilts the faults that matter and leaves the others alone, which no uniform ``sample_scale`` can do.

    Among product-of-Bernoulli rows the one closest (in cross-entropy) to the ideal sampler "the model's faults, given that
    the decoder fails" sets every fault's probability to its likelihood-weighted frequency among the failing shots,
    ``sum_fail w f_i / sum_fail w``.  Failures have to be common for that to be measurable, so the nominal noise walks down:
    with ``scaled(beta)_i = p_i`` where ``p_i >= 0.5``, else ``min(beta p_i, 0.5)``, the fit starts at
    ``q = scaled(levels[0])``, and level t samples ``shots_per_level`` shots from the current q under the nominal row
    ``scaled(levels[t])`` (``set_sampling(q, nominal=...)``, from global shot ``t << 40`` on, as the strata of
    :func:`dem_failure_spectrum`), decodes with ``priors`` and updates

        q_i <- clip((1 - smoothing) q_i + smoothing S_i / S, p_i, 0.5)   where 0 < p_i < 0.5;    q_i = p_i elsewhere

    so that every row on the way is a legal ``sample_priors`` that never samples a fault more rarely than the model does.
    ``S_i`` and ``S`` are summed per batch from integers: with lw the log-weights of the batch's failing shots,
    ``v = weight_multipliers(lw)`` and ``(_, sums) = fault_sums("failing", v)`` -- on engine="native" the device's column
    sums, N numbers per batch in place of the failing rows -- ``S_i += sums_i e^(max lw / 2^32)`` and
    ``S += sum(v) e^(max lw / 2^32)`` in float64, in batch order: both engines return the same array, bit for bit, for the
    same ``batch_size``.  The last level must be 1: the row is fitted for the true priors.

    A level with fewer than ``min_failures`` failing shots is a ValueError that names it.  ``report`` is a list with one dict
    per level: ``level``, ``scale``, ``shots``, ``failures``, ``effective_sample_fraction``, ``weight_mean`` and
    ``sample_priors`` (the row fitted at that level).  ``decoder_kwargs`` go to :class:`dem_decode_sim` (the decoder's
    options, and ``decoder_factory`` with engine="numpy")."""
    levels = [float(b) for b in levels]
    if not levels or not all(1.0 <= b < math.inf for b in levels):
        raise ValueError("levels must be a non-empty sequence of finite scales >= 1")
    if levels[-1] != 1.0:
        raise ValueError(f"the last level must be 1 (the row is fitted for the true priors), not {levels[-1]:g}")
    shots = int(shots_per_level)
    if shots < 1:
        raise ValueError("shots_per_level must be >= 1")
    smoothing = float(smoothing)
    if not 0.0 < smoothing <= 1.0:
        raise ValueError(f"smoothing must be in (0, 1], not {smoothing}")
    min_failures = int(min_failures)
    if min_failures < 1:
        raise ValueError("min_failures must be >= 1")
    for key in ("sample_priors", "sample_scale", "fault_weight", "subset", "support", "harvest", "fault_stats", "target_runs", "run_sim"):
        if key in decoder_kwargs:
            raise ValueError(f"fit_sample_priors sets {key} itself")
    p = checked_model(H, L, priors)[2]
    free = (p > 0.0) & (p < 0.5)
    q = _scaled_priors(p, levels[0])
    sim = dem_decode_sim(H, L, p, batch_size=batch_size, engine=engine, seed=seed, target_runs=shots, run_sim=False, sample_priors=q, harvest=1,
                         **decoder_kwargs)
    run_batch = sim._run_batch_native if engine == "native" else sim._run_batch_numpy
    report = []
    for t, beta in enumerate(levels):
        sim.set_sampling(q, nominal=_scaled_priors(p, beta), target_runs=shots, first_shot=t << 40)
        S_i, S, failures = np.zeros(sim.N, np.float64), 0.0, 0
        while sim.run_count < shots:
            run_batch(min(sim._batch_size, shots - sim.run_count))
            rows = sim.last_batch("fail_rows")
            if not rows.size:
                continue
            lw = sim.last_batch("logw")[rows]
            v = weight_multipliers(lw)
            _, sums = sim.fault_sums("failing", v)
            top = math.exp(int(lw.max()) / LOGW_ONE)
            S_i += sums.astype(np.float64) * top
            S += float(int(v.sum(dtype=np.uint64))) * top
            failures += int(rows.size)
        if failures < min_failures:
            raise ValueError(f"level {t} (scale {beta:g}) saw {failures} failing shots in {shots}, fewer than min_failures = {min_failures}: "
                             "start from a larger first scale, or give every level more shots")
        q = np.where(free, np.clip((1.0 - smoothing) * q + smoothing * (S_i / S), p, 0.5), p)
        report.append({"level": t, "scale": beta, "shots": shots, "failures": failures,
                       "effective_sample_fraction": float(sim.effective_sample_fraction), "weight_mean": float(sim.weight_mean),
                       "sample_priors": q.copy()})
    return q, report
