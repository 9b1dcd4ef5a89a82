"""What the two detector-error-model harnesses share (``dem.dem_decode_sim`` and ``window.windowed_dem_decode_sim``): the
model's validation, the run loop over batches, the counters and rates of a run, and the native engine's plumbing (creating a
``bposd_dem``, fetching an item of the last batch, device bytes and kernel times), and the harvest of failing shots: its host
restatement (``harvest_batch``), which is the definition the device kernels are held against, and what a run accumulates
from it; next to it the restatement of the per-fault sums over selected shots (``fault_sums_batch``).  A harness keeps its constructor, its two ``_run_batch_*`` and what is its own in ``last_batch`` and
``output_dict``."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def _gf2_csr(a, what):
    """scipy CSR over GF(2) with sorted indices and no stored zeros."""
    if sp.issparse(a):
        m = sp.csr_matrix(a).astype(np.int64)
    else:
        arr = np.asarray(a)
        if arr.ndim != 2:
            raise ValueError(f"{what} must be a 2-D array or scipy.sparse matrix")
        m = sp.csr_matrix(arr.astype(np.int64) & 1)
    m.sum_duplicates()
    m.data %= 2
    m.eliminate_zeros()
    m.sort_indices()
    return m.astype(np.uint8)


def _pack(rows):
    """uint8 0/1 rows [B, c] -> uint64 [B, ceil(c/64)] (the C-ABI's packed form)."""
    a = np.ascontiguousarray(rows, dtype=np.uint8)
    by = np.packbits(a, axis=1, bitorder="little")
    out = np.zeros((a.shape[0], 8 * ((a.shape[1] + 63) // 64)), np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u8")


HARVEST_ITEMS = ("fail_rows", "fail_weight", "fail_residual", "fail_faults", "min_residual")


def harvest_batch(faults, correction, select, max_rows):
    """The harvest of one batch on the host -- the definition the device is held against bit for bit.

    ``faults`` and ``correction`` are uint8 0/1 rows [B, N] (of the correction bit 0 counts), ``select`` [B] marks the failing
    shots and ``max_rows`` = K >= 0 caps the rows kept.  With F the selected rows in ascending order and
    ``r_b = faults[b] ^ correction[b]``: ``fail_count`` = |F|, ``fail_rows`` int32 [|F|], ``fail_weight`` int32 [|F|] (the
    weight of r_b for all of F), ``fail_residual`` and ``fail_faults`` uint64 [min(|F|, K), ceil(N/64)] (packed, of the first
    rows of F), ``min_weight`` and ``min_row`` (the least weight over all of F and the lowest row that has it; -1, -1 for an
    empty F) and ``min_residual`` uint64 [ceil(N/64)] (zeros for an empty F)."""
    f = np.asarray(faults, dtype=np.uint8) & 1
    c = np.asarray(correction, dtype=np.uint8) & 1
    rows = np.flatnonzero(np.asarray(select)).astype(np.int32)
    r = f[rows] ^ c[rows]
    weight = r.sum(axis=1, dtype=np.int64).astype(np.int32)
    keep = min(rows.size, int(max_rows))
    out = {"fail_count": int(rows.size), "fail_rows": rows, "fail_weight": weight, "fail_residual": _pack(r[:keep]),
           "fail_faults": _pack(f[rows[:keep]]), "min_weight": -1, "min_row": -1, "min_residual": np.zeros((f.shape[1] + 63) // 64, "<u8")}
    if rows.size:
        i = int(np.argmin(weight))  # the first of the least: rows ascend, so the lowest row
        out.update(min_weight=int(weight[i]), min_row=int(rows[i]), min_residual=_pack(r[i:i + 1])[0])
    return out


def fault_sums_batch(fault_words, rows, multipliers=None, N=None):
    """The per-fault sums over selected shots of one batch on the host -- the definition the device kernel
    (fault_sums_kernel) is held against bit for bit.

    ``fault_words`` are the packed fault rows of a batch, uint64 [B, ceil(N/64)] with padding bits zero (item "faults"),
    ``rows`` an ascending int32 list of F selected rows and ``multipliers`` None or uint32 [F], aligned with ``rows``.
    Returns ``(counts, sums)``, uint64 [N] each (``N`` not given: all 64 ceil(N/64) columns of the words): ``counts[i]`` = the number of
    selected rows in which fault i fired and ``sums[i]`` = the sum of their multipliers (None without multipliers).  All of
    it is integer: no sum can reach 2^63 with multipliers below 2^32 and fewer than 2^31 rows, and every split of the row
    list adds up to the same arrays."""
    words = np.ascontiguousarray(fault_words, dtype="<u8")
    if words.ndim != 2:
        raise ValueError("fault_words must be packed rows [B, ceil(N/64)]")
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    if rows.size and (rows[0] < 0 or rows[-1] >= words.shape[0] or (np.diff(rows) <= 0).any()):
        raise ValueError(f"rows must ascend strictly inside [0, {words.shape[0]})")
    mult = None
    if multipliers is not None:
        mult = np.asarray(multipliers)
        if mult.shape != rows.shape or (mult.size and (not np.issubdtype(mult.dtype, np.integer) or mult.min() < 0 or mult.max() >= 2 ** 32)):
            raise ValueError(f"multipliers must be {rows.size} integers in [0, 2^32), one per selected row")
        mult = mult.astype(np.uint64)
    cols = 64 * words.shape[1]
    N = cols if N is None else int(N)
    if not cols - 64 < N <= cols and not (cols == 0 and N == 0):
        raise ValueError(f"rows of {words.shape[1]} words do not hold N = {N} faults")
    counts, sums = np.zeros(cols, np.uint64), None if mult is None else np.zeros(cols, np.uint64)
    for lo in range(0, rows.size, 4096):  # (unpacked a slab at a time)
        sel = rows[lo:lo + 4096]
        bits = np.unpackbits(np.ascontiguousarray(words[sel]).view(np.uint8), axis=1, bitorder="little")
        counts += bits.sum(axis=0, dtype=np.uint64)
        if mult is not None:
            sums += (bits.astype(np.uint64) * mult[lo:lo + 4096, None]).sum(axis=0, dtype=np.uint64)
    return counts[:N].copy(), None if sums is None else sums[:N].copy()


def checked_model(H, L, priors):
    """``(H, L, priors)`` as GF(2) CSR (M x N), (k x N) and float64 [N], or the ValueError that says what is wrong."""
    H, L = _gf2_csr(H, "H"), _gf2_csr(L, "L")
    N, K = H.shape[1], L.shape[0]
    if L.shape[1] != N:
        raise ValueError(f"L must have shape (k, {N}), not {L.shape}")
    if not 1 <= K <= 4096:
        raise ValueError(f"the number of observables k = {K} is outside 1 .. 4096")
    p = np.ascontiguousarray(priors, dtype=np.float64)
    if p.shape != (N,):
        raise ValueError(f"priors must have length {N}, not {p.shape}")
    bad = np.flatnonzero(~((p >= 0) & (p <= 1)))
    if bad.size:
        raise ValueError(f"the prior of fault {int(bad[0])} ({p[bad[0]]}) is not a probability")
    return H, L, p


def create_dem(lib, device, seed, capacity, H, L, priors, decoder_handle):
    """bposd_dem_create over the model; ``decoder_handle`` None makes a sample-only engine.  Returns the engine pointer."""
    import ctypes as C

    from . import _lib

    cfg = _lib.BposdDemConfig(device=int(device), seed=seed, capacity=int(capacity))
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    keep = [i32(H.indptr), i32(H.indices), i32(L.indptr), i32(L.indices)]
    dem = C.c_void_p()
    rc = lib.bposd_dem_create(C.byref(cfg), decoder_handle, keep[0].ctypes.data, keep[1].ctypes.data, H.shape[0], keep[2].ctypes.data,
                              keep[3].ctypes.data, L.shape[0], H.shape[1], priors.ctypes.data, C.byref(dem))
    _lib.check_dem(lib, None, rc)
    return dem


class DemSimBase:
    """The run of a harness.  A subclass sets ``_COUNTS`` (the counters of a batch, in the library's order), ``_RATES`` (the
    keys whose ``<key>_success_count`` gets a ``<key>_logical_error_rate`` and ``..._eb``), ``M``, ``N`` and ``K``, and has
    ``_run_batch_native(B)`` and ``_run_batch_numpy(B)``, which end in :meth:`_accumulate`."""

    _COUNTS = ()
    _RATES = ()
    _lib = None

    def _check_engine(self, engine, decoder_factory, drives):
        if engine not in ("native", "numpy"):
            raise ValueError("engine must be 'native' or 'numpy'")
        if engine == "native" and decoder_factory is not None:
            raise ValueError(f"engine='native' drives the MI355X {drives} through device pointers; decoder_factory must be None")
        self._engine = self.engine = engine

    def _init_run(self, batch_size, seed, target_runs):
        self._batch_size = int(batch_size)
        if self._batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.seed = int(seed) & (2 ** 64 - 1)
        self.target_runs = int(target_runs)
        self.run_count = 0
        for key in self._COUNTS:
            setattr(self, key, 0)
        for key in self._RATES:
            setattr(self, f"{key}_logical_error_rate", 0.0)
            setattr(self, f"{key}_logical_error_rate_eb", 0.0)
        self._obs_fail = np.zeros(self.K, np.int64)
        self.osdw_observable_error_rates = np.zeros(self.K, np.float64)
        self._last = None  # engine="numpy": the items of the last batch
        self._last_B = 0   # engine="native": its size

    # ------------------------------------------------------------------ the harvest of failing shots
    def _init_harvest(self, harvest, with_logw=False):
        """``harvest=K``: an int >= 0.  Sets the results of a harvest (all None while it is off)."""
        if isinstance(harvest, bool) or not isinstance(harvest, (int, np.integer)) or harvest < 0:
            raise ValueError(f"harvest must be an int >= 0 (the failing shots to keep; 0: off), not {harvest!r}")
        self.harvest = int(harvest)
        self.min_logical_weight = self.min_logical_shot = self.min_logical_fault = None
        self.failure_weight_counts = self.failures = None
        self._last_info = None  # (fail_count, min_weight, min_row, rows asked for) of the last batch
        if self.harvest:
            fw = (self.N + 63) // 64
            self.failure_weight_counts = np.zeros(self.N + 1, np.int64)
            self.failures = {"shot": np.zeros(0, np.uint64), "weight": np.zeros(0, np.int32), "residual": np.zeros((0, fw), "<u8"),
                             "faults": np.zeros((0, fw), "<u8")}
            if with_logw:
                self.failures["logw"] = np.zeros(0, np.int64)

    def _harvest_ask(self):
        """Rows the next batch is asked to keep: the ones still missing of the run's first K (an engine that is on keeps one)."""
        return max(1, self.harvest - self.failures["shot"].size)

    def _set_native_harvest(self, handle, set_fn, check, rows):
        """bposd_*_set_harvest in front of a batch: the engine keeps ``rows`` rows of it."""
        check(self._lib, handle, getattr(self._lib, set_fn)(handle, int(rows)))

    def _native_harvest_triple(self, handle, info_fn, check):
        """bposd_*_harvest_info of the batch that ran: [fail_count, min_weight, min_row]."""
        import ctypes as C

        t = (C.c_int64 * 3)()
        check(self._lib, handle, getattr(self._lib, info_fn)(handle, t))
        return [int(v) for v in t]

    def _accumulate_harvest(self, first_shot, info, ask, logw=None):
        """One batch's harvest into the run's: ``info`` = (fail_count, min_weight, min_row); the items come from
        ``last_batch``, so both engines take the same path."""
        count, min_w, min_row = info
        self._last_info = (count, min_w, min_row, ask)
        if not count:
            return
        rows, weight = self.last_batch("fail_rows"), self.last_batch("fail_weight")
        self.failure_weight_counts += np.bincount(weight, minlength=self.N + 1)
        F = self.failures
        take = min(self.harvest - F["shot"].size, count)
        if take > 0:
            sel = rows[:take]
            F["shot"] = np.concatenate([F["shot"], (np.uint64(first_shot) + sel.astype(np.uint64))])
            F["weight"] = np.concatenate([F["weight"], weight[:take]])
            F["residual"] = np.concatenate([F["residual"], self.last_batch("fail_residual")[:take]])
            F["faults"] = np.concatenate([F["faults"], self.last_batch("fail_faults")[:take]])
            if logw is not None:
                F["logw"] = np.concatenate([F["logw"], np.asarray(logw, dtype=np.int64)[sel]])
        if self.min_logical_weight is None or min_w < self.min_logical_weight:  # (a tie stays with the earlier shot)
            self.min_logical_weight, self.min_logical_shot = int(min_w), int(first_shot) + int(min_row)
            words = np.ascontiguousarray(self.last_batch("min_residual")).reshape(1, -1)
            self.min_logical_fault = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[0, :self.N].copy()

    def _check_harvest_item(self, what):
        if what in HARVEST_ITEMS and not self.harvest:
            raise ValueError(f"last_batch({what!r}) needs harvest=K > 0")

    def run_decode_sim(self):
        while self.run_count < self.target_runs:
            B = min(self._batch_size, self.target_runs - self.run_count)
            if self._engine == "native":
                self._run_batch_native(B)
            else:
                self._run_batch_numpy(B)
        return self.output_dict()

    def _accumulate(self, B, counters, obs_fail):
        self.run_count += B
        for key, v in zip(self._COUNTS, counters):
            setattr(self, key, getattr(self, key) + v)
        self._obs_fail += np.asarray(obs_fail, dtype=np.int64)
        n = self.run_count
        for key in self._RATES:  # css_decode_sim's formulas
            ler = 1 - getattr(self, f"{key}_success_count") / n
            setattr(self, f"{key}_logical_error_rate", ler)
            setattr(self, f"{key}_logical_error_rate_eb", float(np.sqrt((1 - ler) * ler / n)))
        self.osdw_observable_error_rates = self._obs_fail / n

    def _results(self):
        """The part of ``output_dict`` every harness has: the run, its counters, rates and failures per observable."""
        out = {"N": self.N, "M": self.M, "K": self.K, "seed": self.seed, "engine": self.engine, "target_runs": self.target_runs,
               "run_count": self.run_count}
        for key in self._COUNTS:
            out[key] = int(getattr(self, key))
        for key in self._RATES:
            out[f"{key}_logical_error_rate"] = float(getattr(self, f"{key}_logical_error_rate"))
            out[f"{key}_logical_error_rate_eb"] = float(getattr(self, f"{key}_logical_error_rate_eb"))
        out["osdw_observable_error_rates"] = [float(v) for v in self.osdw_observable_error_rates]
        return out

    # ------------------------------------------------------------------ the library's engine
    def _device_bytes(self, handle, fn):
        if handle is None:
            raise RuntimeError("device_bytes needs engine='native'")
        return int(getattr(self._lib, fn)(handle))

    def _kernel_ms(self, handle, fn, check):
        import ctypes as C

        if handle is None:
            raise RuntimeError("kernel_ms needs engine='native'")
        a, b = C.c_double(), C.c_double()
        check(self._lib, handle, getattr(self._lib, fn)(handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _last_batch(self, what, fetch):
        """Item ``what`` (a name the subclass has checked) of the last batch: the numpy engine's array, or ``fetch()``."""
        if self._engine == "numpy":
            if self._last is None:
                raise RuntimeError("last_batch needs a batch that has run")
            return self._last[what]
        if not self._last_B:
            raise RuntimeError("last_batch needs a batch that has run")
        return fetch()

    def _fetch(self, items, handle, fetch_fn, check_fn, what):
        """Entry ``what`` of a ``_lib.*_ITEMS`` table from the engine ``handle``: its shape for the last batch, and the copy."""
        item, dtype, cols = items[what]
        B = self._last_B
        width = {"N": self.N, "M": self.M, "k": self.K}
        if cols in ("F", "FN", "1N"):  # of a harvest: sized by the batch's failures
            if self._last_info is None:
                raise RuntimeError(f"last_batch({what!r}) needs a batch that ran with the harvest on")
            count, _, _, ask = self._last_info
            fw = (self.N + 63) // 64
            shape = (count,) if cols == "F" else (min(count, ask), fw) if cols == "FN" else (fw,)
        else:
            shape = (B,) if cols is None else (self.K,) if cols == "k32" else (B, (width[cols] + 63) // 64)
        out = np.empty(shape, dtype=np.dtype(dtype))
        if out.nbytes == 0:
            return out
        check_fn(self._lib, handle, fetch_fn(handle, item, out.ctypes.data, out.nbytes))
        return out
