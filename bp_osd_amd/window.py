"""Sliding-window decoding of detector error models: the third engine, next to ``dem_decode_sim``.

A model that is decoded as one matrix meets the decoder's limits after a few rounds and its cost per shot grows
with the square of the number of rounds.  A window decoder cuts the model along time: window ``w`` of ``window = (W, C)``
covers the detector times ``[w C, w C + W)``, is decoded on a decoder of its own and *commits* the faults of its first ``C``
times; their columns are XORed out of the running detector row, and the next window decodes what is left.  DESIGN.md 4.12
has the definition; in short, with ``tau_i`` the smallest ``detector_time`` among the detectors of fault ``i``:

    D_w = detectors with time in [lo, hi)          F_w = faults with tau in [lo, hi)
    H_w = H[D_w][:, F_w]                           commit set = faults of F_w with tau < lo + C (the last window: all of F_w)
    per shot: s = r[D_w] -> osdw row c of window w's decoder -> for every committed j with c_j = 1:
              r ^= H[:, F_w[j]],  obs ^= L[:, F_w[j]],  corr[F_w[j]] = 1

Every window must have full row rank (``window_plan`` checks it on the host): the final ``r`` is then zero for every shot.

``WindowedDemDecoder`` decodes detector rows from anywhere; ``windowed_dem_decode_sim`` is the Monte-Carlo harness on
``dem_decode_sim``'s Philox stream.  ``engine="native"`` chains the windows on the device (include/bposd_mi355x.h "Sliding-
window engine"): window_step_kernel commits one window and gathers the next one's syndrome between two decodes, and nothing
but the counters crosses to the host.  ``engine="numpy"`` is the definition above as a host loop around any decoder with a
``decode_batch``; around the CPU oracle it is the reference the device must match bit for bit.
"""
from __future__ import annotations

import json
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from ._dem_base import HARVEST_ITEMS, DemSimBase, _gf2_csr, _pack, checked_model, create_dem, harvest_batch
from .sim import _default_decoder_factory, _mod2_mul, philox_uniforms

__all__ = ["window_plan", "WindowedDemDecoder", "windowed_dem_decode_sim"]

_ITEMS = ("faults", "detectors", "observables", "obs_osdw", "correction", "residual", "flags", "converged", "iters", "obs_fail") + HARVEST_ITEMS


def window_plan(H, detector_time, window, priors=None, check_rank=True, fault_key=None):
    """The index lists of a windowed decode of ``H`` (M x N) with one time per detector and ``window = (W, C)``.

    Returns a namespace with ``M``, ``N``, ``T``, ``W``, ``C``, ``tau`` (int64 [N], -1 for a fault with an empty column) and
    ``windows``: one namespace per window with ``lo``, ``hi``, ``det`` (D_w, int32 ascending), ``fault`` (F_w, int32
    ascending), ``commit`` (uint8 per entry of ``fault``), ``H`` (H_w, CSR uint8) and ``handle`` (index into ``unique``).
    ``unique`` lists the first window of every distinct (H_w, priors_w) -- without ``priors``, of every distinct H_w -- so a
    time-invariant model needs two or three decoders whatever its T.  ``step_words[s] = (w_lo, w_hi)`` for step s = 0 ..
    len(windows): the 64-bit words of the detector row that the columns committed from window s - 1 touch or the gather of
    window s reads, which is all that window_step_kernel stages.  ``fault_key`` (an array with one row per fault, e.g. the
    transposed memory strengths of a relay configuration over all N faults) joins H_w and priors_w in what makes two windows
    distinct: windows share a decoder only where their rows of it agree too.

    ValueError (naming the window) for an empty D_w or F_w and, with ``check_rank``, for rank(H_w) < |D_w|."""
    from .codes import gf2_rank

    H = _gf2_csr(H, "H")
    M, N = H.shape
    try:
        W, C = (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError("window must be a pair (W, C)") from None
    if not 1 <= C <= W:
        raise ValueError(f"window = ({W}, {C}) must have 1 <= C <= W")
    t = np.asarray(detector_time)
    if t.shape != (M,):
        raise ValueError(f"detector_time must have length {M} (one time per detector), not shape {t.shape}")
    if not np.issubdtype(t.dtype, np.integer):
        if not np.all(t == np.floor(t)):
            raise ValueError("detector_time must hold integers")
    t = t.astype(np.int64)
    if t.min() < 0:
        raise ValueError("detector_time must be >= 0")
    T = int(t.max()) + 1
    csc = H.tocsc()
    csc.sort_indices()
    tau = np.full(N, -1, np.int64)
    nonempty = np.flatnonzero(np.diff(csc.indptr))
    if nonempty.size:
        tau[nonempty] = np.minimum.reduceat(t[csc.indices], csc.indptr[nonempty])
    p = None if priors is None else np.ascontiguousarray(priors, dtype=np.float64)
    if p is not None and p.shape != (N,):
        raise ValueError(f"priors must have length {N}, not {p.shape}")
    fk = None if fault_key is None else np.ascontiguousarray(fault_key)
    if fk is not None and (fk.ndim < 1 or fk.shape[0] != N):
        raise ValueError(f"fault_key must have one row per fault ({N}), not shape {fk.shape}")

    windows, unique, seen = [], [], {}
    w = 0
    while True:
        lo, hi = w * C, w * C + W
        last = hi >= T
        det = np.flatnonzero((t >= lo) & (t < hi)).astype(np.int32)
        fault = np.flatnonzero((tau >= lo) & (tau < hi)).astype(np.int32)
        if det.size == 0 or fault.size == 0:
            raise ValueError(f"window {w} (times [{lo}, {hi})) holds {det.size} detectors and {fault.size} faults: a window must have both")
        commit = np.ones(fault.size, np.uint8) if last else (tau[fault] < lo + C).astype(np.uint8)
        Hw = H[det][:, fault].tocsr()
        Hw.sort_indices()
        key = (Hw.shape, Hw.indptr.tobytes(), Hw.indices.tobytes(), b"" if p is None else p[fault].tobytes(),
               b"" if fk is None else fk[fault].tobytes())
        if key not in seen:
            if check_rank:
                rank = gf2_rank(Hw.toarray())
                if rank < det.size:
                    raise ValueError(f"window {w} (times [{lo}, {hi})) is {det.size} x {fault.size} with rank {rank}: every window needs "
                                     "full row rank (drop dependent detectors, DESIGN.md 4.12)")
            seen[key] = len(unique)
            unique.append(w)
        windows.append(SimpleNamespace(index=w, lo=lo, hi=hi, det=det, fault=fault, commit=commit, H=Hw, handle=seen[key]))
        if last:
            break
        w += 1

    step_words = []
    for s in range(len(windows) + 1):
        bits = []
        if s > 0:
            prev = windows[s - 1]
            cols = prev.fault[prev.commit != 0]
            if cols.size:
                bits.append(csc[:, cols].indices)
        if s < len(windows):
            bits.append(windows[s].det)
        bits = np.concatenate(bits) if bits else np.zeros(0, np.int64)
        step_words.append((int(bits.min()) >> 6, (int(bits.max()) >> 6) + 1) if bits.size else (0, 0))
    return SimpleNamespace(M=M, N=N, T=T, W=W, C=C, tau=tau, windows=windows, unique=unique, step_words=step_words, H=H)


def _split_decode(r, decoder):
    """(osdw rows, converged, iters) of a ``decode_batch`` result in either of the forms dem_decode_sim takes."""
    if isinstance(r, dict):
        return np.asarray(r["osdw"]), np.asarray(r["converged"]), np.asarray(r["iters"])
    return np.asarray(r), np.asarray(decoder.batch_converge), np.asarray(decoder.batch_iter)


def _refuse_lsd(decoder_kwargs):
    """LSD mode (``BpOsdDecoder(lsd=...)``) is not offered for windows; without this check the keyword would reach every
    window's decoder unnoticed."""
    if decoder_kwargs.get("lsd") is not None:
        raise ValueError("windowed decoding takes no lsd= argument: LSD mode belongs to the unwindowed decoder (dem_decode_sim)")


class _Model:
    """The validated model and its plan: what both classes below start from."""

    def __init__(self, H, L, priors, detector_time, window, relay=None):
        self.H, self.L, self.priors = checked_model(H, L, priors)
        self.M, self.N = self.H.shape
        self.K = self.L.shape[0]
        # relay= over the model: memory strengths for all N faults, every window takes the columns of its own faults, and
        # windows share a decoder only where those agree (a configuration of another width goes to every window as it is)
        self.relay = relay if relay is not None and getattr(relay, "n", None) == self.N else None
        self.plan = window_plan(self.H, detector_time, window, priors=self.priors,
                                fault_key=None if self.relay is None else self.relay.gammas.T)
        self.HT = self.H.T.tocsr()  # row i = column i of H
        self.LT = self.L.T.tocsr()

    def make_decoders(self, factory, decoder_kwargs):
        """One decoder per distinct window; a refusal of the decoder's own constructor names the window."""
        decs = []
        for w in self.plan.unique:
            win = self.plan.windows[w]
            kw = decoder_kwargs if self.relay is None else dict(decoder_kwargs, relay=self.relay.restrict(win.fault))
            try:
                decs.append(factory(win.H, channel_probs=self.priors[win.fault], **kw))
            except ValueError as e:
                raise ValueError(f"window {w} (times [{win.lo}, {win.hi}), {win.H.shape[0]} x {win.H.shape[1]}): {e}") from None
        return decs

    def decode_host(self, decoders, detectors):
        """The per-shot definition for uint8 detector rows [B, M]: (obs, corr, residual, converged in every window, iters)."""
        r = np.array(detectors, dtype=np.uint8) & 1
        B = r.shape[0]
        obs = np.zeros((B, self.K), np.uint8)
        corr = np.zeros((B, self.N), np.uint8)
        conv = np.ones(B, bool)
        iters = np.zeros(B, np.int64)
        for win in self.plan.windows:
            dec = decoders[win.handle]
            rows, cv, it = _split_decode(dec.decode_batch(np.ascontiguousarray(r[:, win.det])), dec)
            conv &= cv.astype(bool)
            iters += it.astype(np.int64)
            sel = np.flatnonzero(win.commit)
            cols = win.fault[sel]
            c = np.ascontiguousarray(rows[:, sel], dtype=np.uint8) & 1
            r ^= _mod2_mul(self.HT[cols].T.tocsr(), c)
            obs ^= _mod2_mul(self.LT[cols].T.tocsr(), c)
            corr[:, cols] = c
        return obs, corr, r, conv, iters.astype(np.int32)


def _native_engine(model, decoders, device, capacity):
    """bposd_window_create on the plan of ``model`` over GPU decoders; returns (lib, engine pointer)."""
    import ctypes as C

    from . import _lib

    lib = _lib.load()
    plan = model.plan
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    wins = plan.windows
    det_ptr = i32(np.concatenate([[0], np.cumsum([w.det.size for w in wins])]))
    fault_ptr = i32(np.concatenate([[0], np.cumsum([w.fault.size for w in wins])]))
    det, fault = i32(np.concatenate([w.det for w in wins])), i32(np.concatenate([w.fault for w in wins]))
    commit = np.ascontiguousarray(np.concatenate([w.commit for w in wins]), dtype=np.uint8)
    keep = [i32(model.H.indptr), i32(model.H.indices), i32(model.L.indptr), i32(model.L.indices)]
    handles = (C.c_void_p * len(wins))(*[decoders[w.handle]._h for w in wins])
    cfg = _lib.BposdWindowConfig(device=int(device), capacity=int(capacity))
    out = C.c_void_p()
    rc = lib.bposd_window_create(C.byref(cfg), model.M, model.N, model.K, keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data,
                                 keep[3].ctypes.data, len(wins), handles, det_ptr.ctypes.data, det.ctypes.data, fault_ptr.ctypes.data,
                                 fault.ctypes.data, commit.ctypes.data, C.byref(out))
    if rc != 0:
        _lib.check_window(lib, None, rc)
    return lib, out


class WindowedDemDecoder:
    """Windowed decode of detector rows from anywhere (a circuit simulator, an experiment): no sampling, no scoring.

    H, L, priors : the model, as ``dem_decode_sim`` takes it
    detector_time : M integers >= 0, the time of every detector (``phenomenological_detector_times``; INTEGRATION.md says how
        they come out of a detector-error-model file)
    window : (W, C), 1 <= C <= W
    batch_size : rows the engine's device buffers hold; a longer ``decode_batch`` runs in chunks of it (default 4096)
    decoder_kwargs : for every window's ``BpOsdDecoder(H_w, channel_probs=priors[F_w], ...)``.  ``relay=`` takes a
        ``RelayConfig`` over all N faults of the model: window w runs with the columns F_w of its memory strengths

    ``decode_batch(detectors)`` returns the observable rows and leaves ``batch_correction``, ``batch_residual``,
    ``batch_converge`` (BP converged in every window) and ``batch_iter`` (iterations summed over the windows)."""

    def __init__(self, H, L, priors, detector_time, window, batch_size=4096, decoders=None, **decoder_kwargs):
        from .decoder import BpOsdDecoder

        self._win = None
        _refuse_lsd(decoder_kwargs)
        self._model = m = _Model(H, L, priors, detector_time, window, relay=decoder_kwargs.get("relay"))
        self.M, self.N, self.K = m.M, m.N, m.K
        self.plan = m.plan
        self._capacity = int(batch_size)
        if self._capacity < 1:
            raise ValueError("batch_size must be >= 1")
        # decoders=: the list another engine over the same model and options made (they are shared, not copied)
        self.decoders = list(decoders) if decoders is not None else m.make_decoders(BpOsdDecoder, decoder_kwargs)
        if len(self.decoders) != len(m.plan.unique):
            raise ValueError(f"the plan has {len(m.plan.unique)} distinct windows, not {len(self.decoders)}")
        self.device = int(self.decoders[0].device)
        self._lib, self._win = _native_engine(m, self.decoders, self.device, self._capacity)
        self.batch_correction = self.batch_residual = self.batch_converge = self.batch_iter = None

    def __del__(self):
        win, self._win = getattr(self, "_win", None), None
        if win is not None:  # before the decoders it points to go
            self._lib.bposd_window_destroy(win)

    close = __del__

    def device_bytes(self):
        """Bytes of device memory the engine holds (the decoders' workspaces are their own)."""
        return int(self._lib.bposd_window_device_bytes(self._win))

    def decode_batch(self, detectors, packed=False):
        """detectors: uint8 0/1 rows [B, M], or uint64 words [B, ceil(M/64)] (a uint64 array, or ``packed=True``).  Returns
        the observable rows in the same form (uint8 [B, k] or uint64 [B, ceil(k/64)]); the ``batch_*`` rows follow it."""
        from . import _lib

        a = np.asarray(detectors)
        packed = bool(packed) or a.dtype == np.uint64
        dw, ow, fw = (self.M + 63) // 64, (self.K + 63) // 64, (self.N + 63) // 64
        if packed:
            words = np.ascontiguousarray(a, dtype="<u8")
            if words.ndim != 2 or words.shape[1] != dw:
                raise ValueError(f"packed detectors must have shape (B, {dw}), not {words.shape}")
        else:
            if a.ndim != 2 or a.shape[1] != self.M:
                raise ValueError(f"detectors must have shape (B, {self.M}), not {a.shape}")
            words = _pack(a)
        B = words.shape[0]
        obs, corr, res = np.zeros((B, ow), "<u8"), np.zeros((B, fw), "<u8"), np.zeros((B, dw), "<u8")
        conv, iters = np.zeros(B, np.uint8), np.zeros(B, np.int32)
        if B:
            _lib.check_window(self._lib, self._win, self._lib.bposd_window_decode(
                self._win, words.ctypes.data, B, obs.ctypes.data, corr.ctypes.data, res.ctypes.data, conv.ctypes.data, iters.ctypes.data))
        self.batch_converge, self.batch_iter = conv.astype(bool), iters
        if packed:
            self.batch_correction, self.batch_residual = corr, res
            return obs
        unpack = lambda wds, c: np.unpackbits(wds.view(np.uint8), axis=1, bitorder="little")[:, :c]
        self.batch_correction, self.batch_residual = unpack(corr, self.N), unpack(res, self.M)
        return unpack(obs, self.K)

    def decode_batch_device(self, d_detector_words, B, d_obs_words, d_correction_words=None, d_residual_words=None, d_converged=None,
                            d_iters=None, wait=False):
        """Device-pointer form: integers (``tensor.data_ptr()``) of uint64 rows on the engine's device -- detectors [B, ceil(M/64)]
        in, observables [B, ceil(k/64)] out, optionally correction [B, ceil(N/64)], residual [B, ceil(M/64)], converged uint8
        [B], iters int32 [B].  B <= batch_size.  Asynchronous on the engine's stream: ``synchronize()`` (or ``wait=True``)
        before the outputs are read; the engine's stream is not the caller's, so the inputs must be complete at the call."""
        from . import _lib

        z = lambda v: None if v is None else int(v)
        _lib.check_window(self._lib, self._win, self._lib.bposd_window_decode_device(
            self._win, int(d_detector_words), int(B), int(d_obs_words), z(d_correction_words), z(d_residual_words), z(d_converged), z(d_iters)))
        if wait:
            self.synchronize()

    def synchronize(self):
        from . import _lib

        _lib.check_window(self._lib, self._win, self._lib.bposd_window_synchronize(self._win))

    def kernel_ms(self):
        """(sum of the window_step_kernel launches, window_score_kernel) of the last batch in ms (HIP events)."""
        import ctypes as C

        from . import _lib

        a, b = C.c_double(), C.c_double()
        _lib.check_window(self._lib, self._win, self._lib.bposd_debug_window_timing(self._win, C.byref(a), C.byref(b)))
        return a.value, b.value


class windowed_dem_decode_sim(DemSimBase):
    """Monte-Carlo harness of the windowed decoder; see the module docstring.

    H, L, priors, detector_time, window : as ``WindowedDemDecoder`` takes them
    batch_size : shots per batch (default 4096)
    engine : "native" (sample, windows and scoring in the library; one ``BpOsdDecoder`` per distinct window) or "numpy" (the
        per-shot definition as a host loop around ``decoder_factory(H_w, channel_probs=priors[F_w], **decoder_kwargs)``)
    seed, target_runs, run_sim : as in ``dem_decode_sim``; the Philox stream is the same one, so both engines and the
        unwindowed harness see the same shots
    decoder_factory : engine="numpy" only; default the MI355X ``BpOsdDecoder``
    harvest : K >= 0, as in ``dem_decode_sim``; a shot fails here when its observables are wrong and its final residual
        detector row is zero, and the residual fault set is ``faults ^ correction`` (no "logw": the window run is unweighted)

    Results: ``run_count``, ``bp_converge_count`` (BP converged in every window), ``osdw_success_count`` (observables right),
    ``residual_count`` (final detector row not zero: 0 for full-rank windows), ``trivial_count`` (no detector fired),
    ``osdw_logical_error_rate`` with ``osdw_logical_error_rate_eb``, ``osdw_observable_error_rates`` (float [k]),
    :meth:`last_batch` and :meth:`output_dict`."""

    _COUNTS = ("bp_converge_count", "osdw_success_count", "residual_count", "trivial_count")
    _RATES = ("osdw",)

    def __init__(self, H, L, priors, detector_time, window, batch_size=4096, engine="native", seed=0, target_runs=100,
                 decoder_factory=None, run_sim=True, harvest=0, **decoder_kwargs):
        self._check_engine(engine, decoder_factory, "decoders")
        self._win = self._sampler = None
        _refuse_lsd(decoder_kwargs)
        self._model = m = _Model(H, L, priors, detector_time, window, relay=decoder_kwargs.get("relay"))
        self.M, self.N, self.K = m.M, m.N, m.K
        self._init_harvest(harvest)
        self.plan = m.plan
        self._init_run(batch_size, seed, target_runs)
        if engine == "native":
            from .decoder import BpOsdDecoder

            self.decoders = m.make_decoders(BpOsdDecoder, decoder_kwargs)
            self._native_setup()
        else:
            self.decoders = m.make_decoders(decoder_factory or _default_decoder_factory, decoder_kwargs)
        if run_sim:
            self.run_decode_sim()

    # ------------------------------------------------------------------ the library's engine
    def _native_setup(self):
        m = self._model
        device = int(self.decoders[0].device)
        self._lib, self._win = _native_engine(m, self.decoders, device, self._batch_size)
        self._sampler = create_dem(self._lib, device, self.seed, self._batch_size, m.H, m.L, m.priors, None)  # a sample-only engine

    def _run_batch_native(self, B):
        import ctypes as C

        from . import _lib

        c = (C.c_int64 * 4)()
        first, ask = self.run_count, None
        if self.harvest:
            ask = self._harvest_ask()
            self._set_native_harvest(self._win, "bposd_window_set_harvest", _lib.check_window, ask)
        _lib.check_window(self._lib, self._win, self._lib.bposd_window_run(self._win, self._sampler, int(first), int(B), c))
        self._last_B = B
        self._accumulate(B, [int(v) for v in c], self.last_batch("obs_fail"))
        if self.harvest:
            info = self._native_harvest_triple(self._win, "bposd_window_harvest_info", _lib.check_window)
            self._accumulate_harvest(first, info, ask)

    def device_bytes(self):
        """engine="native": bytes of device memory the window engine holds (sampler and decoders hold their own)."""
        return self._device_bytes(self._win, "bposd_window_device_bytes")

    def kernel_ms(self):
        """engine="native": (sum of the window_step_kernel launches, window_score_kernel) of the last batch in ms."""
        from . import _lib

        return self._kernel_ms(self._win, "bposd_debug_window_timing", _lib.check_window)

    def __del__(self):
        win, self._win = getattr(self, "_win", None), None
        if win is not None:  # before the decoders and the sampler it reads
            self._lib.bposd_window_destroy(win)
        dem, self._sampler = getattr(self, "_sampler", None), None
        if dem is not None:
            self._lib.bposd_dem_destroy(dem)

    # ------------------------------------------------------------------ the host loop
    def _run_batch_numpy(self, B):
        m = self._model
        faults = (philox_uniforms(self.seed, self.run_count, B, m.N) < m.priors).astype(np.uint8)
        detectors = _mod2_mul(m.H, faults)
        truth = _mod2_mul(m.L, faults)
        obs, corr, res, conv, iters = m.decode_host(self.decoders, detectors)
        wrong = (obs != truth).any(axis=1)
        dirty = res.any(axis=1)
        quiet = ~detectors.any(axis=1)
        flags = wrong.astype(np.uint8) | (dirty.astype(np.uint8) << 1) | (quiet.astype(np.uint8) << 3)
        obs_fail = (obs != truth).sum(axis=0).astype(np.int32)
        self._last = {"faults": _pack(faults), "detectors": _pack(detectors), "observables": _pack(truth), "obs_osdw": _pack(obs),
                      "correction": _pack(corr), "residual": _pack(res), "flags": flags, "converged": conv.astype(np.uint8), "iters": iters,
                      "obs_fail": obs_fail}
        first = self.run_count
        self._accumulate(B, [int(conv.sum()), int((~wrong).sum()), int(dirty.sum()), int(quiet.sum())], obs_fail)
        if self.harvest:  # observables wrong on a residual of zero, against the committed correction
            ask = self._harvest_ask()
            h = harvest_batch(faults, corr, wrong & ~dirty, ask)
            self._last.update({item: h[item] for item in HARVEST_ITEMS})
            self._accumulate_harvest(first, (h["fail_count"], h["min_weight"], h["min_row"]), ask)

    # ------------------------------------------------------------------ common
    def last_batch(self, what):
        """One array of the last batch: "faults", "detectors", "observables" (the true ones), "obs_osdw", "correction",
        "residual" (bit-packed rows, uint64 [B, ceil(./64)]), "flags" (uint8 [B]: bit 0 observables wrong, bit 1 residual not
        zero, bit 3 no detector fired), "converged" (uint8 [B]: in every window), "iters" (int32 [B]: summed over the windows)
        or "obs_fail" (int32 [k]); with ``harvest=K`` the five items of a harvest as ``dem_decode_sim.last_batch`` has them."""
        from . import _lib

        if what not in _ITEMS:
            raise ValueError(f"what must be one of {sorted(_ITEMS)}")
        self._check_harvest_item(what)
        if what in ("faults", "detectors"):  # the sampler's own rows
            return self._last_batch(what, lambda: self._fetch(_lib.DEM_ITEMS, self._sampler, self._lib.bposd_dem_fetch, _lib.check_dem, what))
        return self._last_batch(what, lambda: self._fetch(_lib.WINDOW_ITEMS, self._win, self._lib.bposd_window_fetch, _lib.check_window, what))

    def output_dict(self):
        """The counters and rates as a JSON string (as dem_decode_sim.output_dict returns one)."""
        out = dict(self._results(), T=self.plan.T, window=[self.plan.W, self.plan.C], windows=len(self.plan.windows), decoders=len(self.plan.unique))
        if self.harvest:
            out["min_logical_weight"] = self.min_logical_weight
        return json.dumps(out, sort_keys=True, indent=4)
