/*
 * bposd_mi355x.h -- C-ABI of libbposd_mi355x.so, the MI355X (gfx950) BP+OSD decoder.
 *
 * This is the drop-in boundary for the reference's decode path.  The reference has
 * no C/FFI plugin interface of its own: its "operator API" is the Python class
 * `bposd_decoder` / `BpOsdDecoder` that it imports from the third-party `ldpc`
 * package (/root/reference/src/bposd/__init__.py:1,
 * /root/reference/src/bposd/css_decode_sim.py:6).  Each entry point below names the
 * reference interface it replaces; bp_osd_amd/decoder.py binds them with ctypes and
 * re-creates that Python class on top (INTEGRATION.md shows the one-line switch).
 *
 * Plain C: opaque handle, plain pointers and sizes, no C++ or torch types.
 * Return value 0 = OK, negative = error (message via bposd_last_error).  The library
 * never aborts the process.  One handle <-> one device <-> one caller thread at a
 * time; different handles may be driven from different threads.
 */
#ifndef BPOSD_MI355X_H
#define BPOSD_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)

typedef struct bposd_handle bposd_handle;

/* Values of bposd_config fields. */
enum { BPOSD_BP_PRODUCT_SUM = 0, BPOSD_BP_MIN_SUM = 1 };
enum { BPOSD_OSD_OFF = 0, BPOSD_OSD_0 = 1, BPOSD_OSD_E = 2, BPOSD_OSD_CS = 3 };

/* Error codes. */
enum {
    BPOSD_OK = 0,
    BPOSD_ERR_INVALID = -1,     /* bad argument / shape / option          -> ValueError   */
    BPOSD_ERR_UNSUPPORTED = -2, /* valid request this build cannot run    -> ValueError   */
    BPOSD_ERR_HIP = -3,         /* HIP runtime failure                    -> RuntimeError */
    BPOSD_ERR_NO_DEVICE = -4    /* no gfx950 device visible               -> RuntimeError */
};

/*
 * Constructor options.  Replaces the kwargs of
 *   bposd_decoder(pcm, error_rate, max_iter, bp_method, ms_scaling_factor,
 *                 channel_probs, osd_method, osd_order)      /root/reference/README.md:178-187
 *   BpOsdDecoder(pcm, channel_probs=..., max_iter=..., bp_method=...,
 *                ms_scaling_factor=..., osd_method=..., osd_order=...)
 *                                         /root/reference/src/bposd/css_decode_sim.py:444-463
 */
typedef struct {
    int32_t device;            /* HIP device ordinal (>= 0)                                  */
    int32_t bp_method;         /* BPOSD_BP_*                                                 */
    double ms_scaling_factor;  /* 0 => variable scaling 1 - 2^-it (README.md:184)            */
    int32_t max_iter;          /* 0 => block length n                                        */
    int32_t osd_method;        /* BPOSD_OSD_*                                                */
    int32_t osd_order;         /* osd_e: patterns on the first w non-pivots; osd_cs: pair span */
    int32_t sort_tie_policy;   /* 0 = stable ascending index among equal LLRs, 1 = descending */
    int32_t weight_fn;         /* 0 = sum log(1/p_i) (ldpc v2), 1 = Hamming weight (ldpc v1)  */
    int32_t schedule;          /* 0 = parallel (flooding) BP schedule -- what the reference runs; 1 = ldpc's
                                  "serial" schedule (bits in ascending index).  Was a reserved
                                  word: a zero-filled old config means parallel                */
    double ps_clip;            /* product-sum only.  0 = upstream behaviour: no clipping, so check->bit messages
                                  reach +-inf once tanh rounds to 1 and NaN follows;
                                  C > 0 = every check->bit message is clamped to [-C, C] (build-owned switch,
                                  DESIGN.md "Product-sum").  Occupies two of the four formerly reserved words: a
                                  zero-filled old config means "no clipping"                  */
    int32_t osd_e_bit_order;   /* osd_e: which T position bit b of pattern i = 1 .. 2^w - 1 stands for.  0 = position b
                                  (LSB first; the restatement's reading of upstream), 1 = position
                                  w - 1 - b.  Only the tie between equally light patterns depends on it (the first one
                                  enumerated wins).  An UNVERIFIED-upstream-behaviour switch like sort_tie_policy /
                                  weight_fn; was reserved[0]: a zero-filled old config means LSB first */
    int32_t ps_math_form;      /* product-sum: evaluation order of the check update (bp_osd_amd/csrc/portable_math.h).  0 =
                                  the reference's operation order -- tanh(b2c / 2), then log of the rounded quotient
                                  (1 + x) / (1 - x): four divisions per edge; closest to the platform libm the reference calls
                                  (188 of 2048 clipped BASELINE configs[2] shots differ from it in an integer output).  1 = two
                                  divisions per edge (pm_tanh_half, pm_log_quot): 1.4 x the throughput, 207 of 2048.  Was
                                  reserved[0]: a zero-filled old config means the reference order */
} bposd_config;

/* Number of visible HIP devices (0 if none / runtime unavailable). */
int bposd_device_count(void);

/* Library version string, e.g. "bposd_mi355x 0.1 (gfx950)". */
const char *bposd_version(void);

/*
 * Create a decoder.  pcm is CSR (indptr[m+1], indices[E], column indices strictly
 * ascending within a row); channel_probs[n] are the per-bit error probabilities
 * (`channel_probs`, or `error_rate` broadcast: README.md:180-181).  The library
 * copies everything; the caller keeps ownership of its arrays.
 * Replaces: the ctor call sites README.md:178-187, css_decode_sim.py:444-463.
 */
int bposd_create(const bposd_config *cfg, const int32_t *csr_indptr, const int32_t *csr_indices,
                 int32_t m, int32_t n, const double *channel_probs, bposd_handle **out);

/* Replaces `.update_channel_probs(p)` -- css_decode_sim.py:229,248. */
int bposd_update_channel_probs(bposd_handle *h, const double *channel_probs);

/*
 * Decode B syndromes held in HOST memory (row-major uint8[B*m], values 0/1) and write
 * the results to HOST buffers.  Synchronous.  osdw is required; osd0, bp, converged,
 * iters, llr may be NULL.
 *   osdw[B*n]  -> `.osdw_decoding`  (README.md:202; css_decode_sim.py:257-258)
 *   osd0[B*n]  -> `.osd0_decoding`  (css_decode_sim.py:294-295)
 *   bp[B*n]    -> `.bp_decoding`    (css_decode_sim.py:338-339)
 *   converged[B] -> `.converge`     (css_decode_sim.py:331-336)
 *   iters[B]   -> `.iter`;  llr[B*n] -> `.log_prob_ratios` (final BP LLRs, fp64)
 * Replaces: `.decode(syndrome)` -- README.md:197; css_decode_sim.py:174-202 (B = 1),
 * and is the batched form the MI355X path is built around.
 * A syndrome outside the column space of H (rank-deficient H) has no exact solution: BP's outputs are unaffected, and
 * osd0 is then a solution of the checks of the pivot rows the OSD kernel kept.  Which rows those are is the kernel's
 * choice -- not the reference's partial pivoting, so other checks may stay unsatisfied than there -- but it is the same
 * on every run, and osdw is the candidate search from that osd0: the reference's OSD on the syndrome H osd0, with the
 * same LLRs, returns the same osd0 and osdw.  Inside the column space every output is the reference's.
 */
int bposd_decode_batch(bposd_handle *h, const uint8_t *syndromes, int64_t B, uint8_t *osdw,
                       uint8_t *osd0, uint8_t *bp, uint8_t *converged, int32_t *iters, double *llr);

/*
 * The same call with bit-packed rows (host memory): syndromes as B rows of ceil(m/64) little-endian 64-bit words, osdw /
 * osd0 / bp as B rows of ceil(n/64) words -- bit (i & 63) of word (i >> 6) of a row is entry i, padding bits are zero
 * (numpy: np.packbits(rows, axis=1, bitorder="little") padded to a multiple of 8 bytes).  One eighth of the bytes cross
 * PCIe; the device unpacks the syndromes in front of the BP kernel and packs the result rows behind it.  This is the
 * form SURVEY.md 8(d)(i) / 8(e) recommend for the host-to-host metric.  osd0_words, bp_words, converged, iters may be
 * NULL.  Synchronous.  Replaces the same call sites as bposd_decode_batch.
 */
int bposd_decode_batch_packed(bposd_handle *h, const uint64_t *syndrome_words, int64_t B, uint64_t *osdw_words,
                              uint64_t *osd0_words, uint64_t *bp_words, uint8_t *converged, int32_t *iters);

/*
 * Asynchronous forms of bposd_decode_batch / bposd_decode_batch_packed for a STREAM of batches: the whole call -- upload,
 * kernels, download -- is enqueued on the handle's next lane (see "Lanes" below) and the function returns; consecutive
 * calls overlap on the device, which a synchronous call cannot (it pays its own upload, its longest-running syndrome and
 * its download).  The buffers should come from bposd_host_alloc (with pageable memory the copies block) and must stay
 * untouched until bposd_synchronize_lane(h, lane) with lane = bposd_last_lane(h) read right after the call, or
 * bposd_synchronize(h).  At most bposd_num_lanes(h) calls are in flight; a further call queues behind the oldest.
 * (No counterpart in the reference: its decode is synchronous.)
 */
int bposd_decode_batch_async(bposd_handle *h, const uint8_t *syndromes, int64_t B, uint8_t *osdw, uint8_t *osd0,
                             uint8_t *bp, uint8_t *converged, int32_t *iters, double *llr);
int bposd_decode_batch_packed_async(bposd_handle *h, const uint64_t *syndrome_words, int64_t B, uint64_t *osdw_words,
                                    uint64_t *osd0_words, uint64_t *bp_words, uint8_t *converged, int32_t *iters);

/*
 * Same, but every pointer is a DEVICE pointer on the handle's device (inputs already
 * resident in HBM).  Asynchronous on the handle's stream: call bposd_synchronize()
 * before reading the outputs.
 */
int bposd_decode_batch_device(bposd_handle *h, const uint8_t *d_syndromes, int64_t B,
                              uint8_t *d_osdw, uint8_t *d_osd0, uint8_t *d_bp,
                              uint8_t *d_converged, int32_t *d_iters, double *d_llr);

/* The device-pointer call with bit-packed rows (the layout of bposd_decode_batch_packed; every pointer a device pointer):
 * the kernels read packed syndromes and write packed result rows themselves -- no pack kernel between the decode and the
 * multi-GPU gather (the HBM-resident kernels included, since round 5).  Codes on the any-degree BP kernel or with the serial
 * schedule return BPOSD_ERR_UNSUPPORTED: there bposd_decode_batch_device + bposd_pack_rows_device do the same.
 * Asynchronous like bposd_decode_batch_device. */
int bposd_decode_batch_device_packed(bposd_handle *h, const uint64_t *d_syndrome_words, int64_t B, uint64_t *d_osdw_words,
                                     uint64_t *d_osd0_words, uint64_t *d_bp_words, uint8_t *d_converged, int32_t *d_iters);

/*
 * Per-syndrome channel, two values per bit: bit i of syndrome b is decoded with probability
 * channel_probs_alt[i] where select[b*n + i] != 0 and with the handle's channel_probs[i] elsewhere
 * (BP priors and OSD-W weights alike).  This is exactly what the reference's per-shot Bayesian channel
 * update produces -- /root/reference/src/bposd/css_decode_sim.py:207-248 sets, per shot,
 * p_i = py/(px+py) where the first decoder flipped bit i and pz/(1-px-py) elsewhere, then calls
 * `.update_channel_probs(p)` before the second `.decode` -- batched over B shots.
 * Host-pointer form, synchronous; `select` and `channel_probs_alt` are required here.
 */
int bposd_decode_batch_select(bposd_handle *h, const uint8_t *syndromes, int64_t B,
                              const uint8_t *select, const double *channel_probs_alt, uint8_t *osdw,
                              uint8_t *osd0, uint8_t *bp, uint8_t *converged, int32_t *iters,
                              double *llr);

/* Device-pointer form of the above (d_select on the device; channel_probs_alt stays a HOST array of n
 * doubles, it is uploaded by the call).  Asynchronous like bposd_decode_batch_device. */
int bposd_decode_batch_select_device(bposd_handle *h, const uint8_t *d_syndromes, int64_t B,
                                     const uint8_t *d_select, const double *channel_probs_alt,
                                     uint8_t *d_osdw, uint8_t *d_osd0, uint8_t *d_bp,
                                     uint8_t *d_converged, int32_t *d_iters, double *d_llr);

/*
 * What the kernels read of a channel: prior_llr[i] = log((1 - p_i) / p_i) and cost[i] = log(1 / p_i) for count
 * probabilities, with the host's libm -- the one routine behind bposd_create, bposd_update_channel_probs, the alternative
 * channel of the select calls and the rows of the calls below, so all of them agree bit for bit.  Host only: no handle, no
 * device.  Either output may be NULL.  BPOSD_ERR_INVALID (text: bposd_last_error(NULL)) for a value outside [0, 1] or a NaN;
 * nothing is written then.
 */
int bposd_channel_tables(const double *probs, int64_t count, double *prior_llr, double *cost);

/*
 * A channel of its own for every syndrome: syndrome b is decoded with the error probabilities
 * channel_probs_rows[b*n .. b*n + n) (BP priors and OSD-W weights alike), exactly as
 * `.update_channel_probs(row b)` followed by `.decode(syndrome b)` would -- soft-information readout, graded erasures,
 * drifting noise, windowed decoding.  The rows replace the handle's channel for this call only; the handle's own tables
 * and its alternative channel are untouched.  Host-pointer form, synchronous, same outputs as bposd_decode_batch_select.
 * Every value is validated before anything is enqueued (the error text names the first offending shot and bit); the rows
 * are converted chunk by chunk on a few host threads and staged per lane as fp64 prior rows plus, where the OSD stage
 * weighs candidates with the channel (osd_e / osd_cs of order > 0 with weight_fn 0), fp64 weight rows.  Not offered
 * together with select, nor in the bit-packed form.
 */
int bposd_decode_batch_rows(bposd_handle *h, const uint8_t *syndromes, int64_t B, const double *channel_probs_rows,
                            uint8_t *osdw, uint8_t *osd0, uint8_t *bp, uint8_t *converged, int32_t *iters, double *llr);

/* Device-pointer form: d_prior_llr_rows and d_cost_rows are [B, n] doubles on the device as bposd_channel_tables makes them
 * (d_cost_rows may be NULL where the OSD stage does not weigh candidates, see above, and no sweep of LSD mode is set -- a
 * handle with LSD mode on and BPOSD_LSD_CS / _E weighs with the shot's row whatever the OSD method; it is required otherwise).  The caller
 * owns the rows and keeps them unchanged until the call's lane is synchronised.  Asynchronous like bposd_decode_batch_device. */
int bposd_decode_batch_rows_device(bposd_handle *h, const uint8_t *d_syndromes, int64_t B, const double *d_prior_llr_rows,
                                   const double *d_cost_rows, uint8_t *d_osdw, uint8_t *d_osd0, uint8_t *d_bp,
                                   uint8_t *d_converged, int32_t *d_iters, double *d_llr);

/*
 * Bit-pack B rows of n 0/1 bytes (device) into B rows of ceil(n/64) little-endian 64-bit words (device):
 * bit (i & 63) of word (i >> 6) of row b = d_bytes[b*n + i] & 1.  Used to shrink the one exchange step of
 * the multi-GPU path (the gather of corrections) 8x.  Asynchronous on the handle's stream.
 */
int bposd_pack_rows_device(bposd_handle *h, const uint8_t *d_bytes, int64_t B, int32_t n,
                           uint64_t *d_words);
/* The same on a given lane.  bposd_pack_rows_device queues the kernel on the lane of the MOST RECENT device-pointer
 * decode: it must be called before the next decode call is enqueued, or the rows of an earlier call would be packed on a
 * stream that is not ordered behind the kernel still writing them.  A caller that packs later passes the lane its decode
 * ran on (bposd_last_lane right after that call). */
int bposd_pack_rows_device_lane(bposd_handle *h, int32_t lane, const uint8_t *d_bytes, int64_t B, int32_t n,
                                uint64_t *d_words);

/*
 * Logical observables.  What most callers ask of a correction is which logical observables it flips: observable j of a row
 * is the parity of popcount(L_j & row) for a k x n matrix L over GF(2) (the logical operators of a code, the observable
 * rows of a detector error model).  With a table set, the calls below decode as the calls above do and return, per shot
 * and per output, ceil(k/64) words instead of a row of n bits: bit (j & 63) of word (j >> 6) is observable j, padding bits
 * are zero.  The rows themselves stay on the device, in buffers the lane owns, and obs_kernel runs behind the OSD kernel
 * on the lane's stream.  (No counterpart in the reference: its callers multiply by the logicals themselves,
 * css_decode_sim.py:257-272.)
 *
 * bposd_observable_table: L as CSR (indptr[k+1], indices, columns strictly ascending within a row) -> the table the kernel
 * reads, table[ceil(n/64)][k] (transposed and packed: bit (c & 63) of table[(c >> 6) * k + j] = L[j][c]).  Host only: no
 * handle, no device.  BPOSD_ERR_INVALID (text: bposd_last_error(NULL)) for k outside 1 .. 4096, a column outside [0, n) or
 * columns that do not ascend strictly; nothing is written then.
 * bposd_set_observables: copies a table for this handle's n to the device; it replaces any earlier table once every lane
 * has drained.  k = 0 removes it (table may be NULL then).
 */
int bposd_observable_table(const int32_t *indptr, const int32_t *indices, int32_t k, int32_t n, uint64_t *table);
int bposd_set_observables(bposd_handle *h, const uint64_t *table, int32_t k);

/* obs_kernel alone on caller-owned device rows of this handle's n bits -- packed != 0: uint64[B][ceil(n/64)] in the layout of
 * bposd_decode_batch_packed (padding bits zero), else uint8[B][n] (bit 0 of every byte) -- into d_obs_words
 * [B][ceil(k/64)], on a given lane: ordered like bposd_pack_rows_device_lane. */
int bposd_observables_device_lane(bposd_handle *h, int32_t lane, const void *d_rows, int32_t packed, int64_t B,
                                  uint64_t *d_obs_words);

/* Device-pointer decode to observables.  d_syndromes holds uint8[B][m], or (syndromes_packed != 0) uint64[B][ceil(m/64)];
 * either form works on every handle.  d_obs_osdw [B][ceil(k/64)] is required; d_obs_osd0, d_obs_bp, d_converged and d_iters
 * may be NULL.  Takes the handle's next lane and is asynchronous like bposd_decode_batch_device (see "Lanes" below).
 * Without a table every decode call of this group returns BPOSD_ERR_INVALID; B = 0 is a valid call that does nothing. */
int bposd_decode_batch_observables_device(bposd_handle *h, const void *d_syndromes, int32_t syndromes_packed, int64_t B,
                                          uint64_t *d_obs_osdw, uint64_t *d_obs_osd0, uint64_t *d_obs_bp,
                                          uint8_t *d_converged, int32_t *d_iters);

/* Host-pointer forms: syndromes as uint8[B*m] or (_packed) as B rows of ceil(m/64) words.  The synchronous calls run in
 * chunks over the lanes like bposd_decode_batch; per chunk the syndromes go up and ceil(k/64) words per shot and requested
 * output, the flags and the iteration counts come down.  The _async forms enqueue the whole call on the next lane under
 * the rules of bposd_decode_batch_async. */
int bposd_decode_batch_observables(bposd_handle *h, const uint8_t *syndromes, int64_t B, uint64_t *obs_osdw,
                                   uint64_t *obs_osd0, uint64_t *obs_bp, uint8_t *converged, int32_t *iters);
int bposd_decode_batch_observables_packed(bposd_handle *h, const uint64_t *syndrome_words, int64_t B, uint64_t *obs_osdw,
                                          uint64_t *obs_osd0, uint64_t *obs_bp, uint8_t *converged, int32_t *iters);
int bposd_decode_batch_observables_async(bposd_handle *h, const uint8_t *syndromes, int64_t B, uint64_t *obs_osdw,
                                         uint64_t *obs_osd0, uint64_t *obs_bp, uint8_t *converged, int32_t *iters);
int bposd_decode_batch_observables_packed_async(bposd_handle *h, const uint64_t *syndrome_words, int64_t B,
                                                uint64_t *obs_osdw, uint64_t *obs_osd0, uint64_t *obs_bp,
                                                uint8_t *converged, int32_t *iters);

/* Wait for all work queued on the handle (every lane, see below). */
int bposd_synchronize(bposd_handle *h);

/*
 * Lanes.  A handle owns bposd_num_lanes(h) HIP streams with their own workspaces and uses them in turn: consecutive
 * device-pointer calls (and the chunks of one host-pointer call) overlap on the device, so the next call's workgroups
 * take over the CUs that the previous call's last max_iter stragglers and its OSD kernel leave idle.  Consequences
 * for a caller of the asynchronous device-pointer API: two consecutive calls are NOT ordered against each other (give
 * them different output buffers, or synchronise in between); a call is ordered behind the call bposd_num_lanes(h)
 * calls earlier (same lane).  bposd_last_lane() names the lane of the last device-pointer call; bposd_synchronize_lane() waits
 * for that lane only; bposd_lane_timing() is bposd_last_timing() for the last call queued on one lane.
 * (No counterpart in the reference: its decoder is a synchronous single-thread object.)
 */
int bposd_num_lanes(bposd_handle *h); /* lanes this handle cycles through (4; 2 for HBM-resident codes); NULL: the maximum */
int bposd_last_lane(bposd_handle *h);
int bposd_synchronize_lane(bposd_handle *h, int32_t lane);
int bposd_lane_timing(bposd_handle *h, int32_t lane, double *bp_ms, double *osd_ms, int64_t *bp_iterations,
                      int64_t *osd_invocations);

/*
 * Page-locked host memory for the host-pointer API: with buffers from here bposd_decode_batch's chunked uploads and
 * downloads are truly asynchronous (pageable memory works too; the host thread then blocks inside each copy).
 * Returns NULL on failure.
 */
void *bposd_host_alloc(size_t bytes);
void bposd_host_free(void *p);

/*
 * Timing and work counters of the LAST decode call, measured with HIP events on the
 * stream the kernels were launched on (waits for that call to finish):
 *   bp_ms, osd_ms    kernel durations (a host-pointer call runs in chunks: the sum over its chunks, which
 *                    overlap on the device; a host-pointer call of up to 1 MB of staging -- the one-syndrome
 *                    decode -- runs without events and reports 0.0 for both)
 *   bp_iterations    sum over syndromes of BP iterations executed
 *   osd_invocations  syndromes that went through OSD (BP did not converge)
 * Any pointer may be NULL.
 */
int bposd_last_timing(bposd_handle *h, double *bp_ms, double *osd_ms, int64_t *bp_iterations,
                      int64_t *osd_invocations);

/* Decoder facts: rank of the pcm over GF(2), number of OSD-W candidates per decode,
 * effective max_iter, nonzeros E.  Any pointer may be NULL. */
int bposd_info(bposd_handle *h, int32_t *rank, int32_t *num_candidates, int32_t *max_iter,
               int32_t *nnz);

/* BP only: posterior log-likelihood ratios (and, optionally, BP's hard decisions, converge flags and iteration counts) of
 * B host syndromes, without the OSD stage whatever osd_method the handle was created with.  This is what the
 * `log_prob_ratios` attribute of the reference's decoder object holds after a decode (SURVEY.md 8 b); the Python class
 * calls it when the attribute is read after a `decode()` that did not ask for LLRs.  llr [B, n] required; bp [B, n], conv
 * [B], iters [B] nullable.  Synchronous. */
int bposd_posterior_llr(bposd_handle *h, const uint8_t *syndromes, int64_t B, double *llr, uint8_t *bp,
                        uint8_t *converged, int32_t *iters);

/* Tuning / test knob for the small-code OSD stage: 0 = auto, 1 = one workgroup per elimination (osd_kernel.hip.h),
 * 2 = one wave per elimination (osd_wave_kernel.hip.h) where it applies (uniform channel, m <= 448, n <= 959, osd_e order
 * <= 12; auto picks it there for calls of at least 4096 syndromes -- a lone elimination is faster on a workgroup of its own).
 * Identical results.  bposd_last_osd_kernel: 1 / 2 as above, 3 = the HBM-resident kernel,
 * -1 before the first OSD launch. */
int bposd_set_osd_variant(bposd_handle *h, int32_t variant);
int bposd_last_osd_kernel(bposd_handle *h);

/* Tuning knob (not part of the reference surface): which BP kernel / workgroup shape runs.
 * 0 = auto; 1, 2, 4 = LDS kernel with 1 / 2 / 4 checks per thread; 16, 17, 18 = local-edge kernel (a third of the
 * messages in registers; (3,6)-regular codes with n = 2m and min-sum only, BPOSD_ERR_UNSUPPORTED otherwise):
 * 2 checks per thread at <= 80 / <= 64 VGPRs, 1 check per thread.  Auto picks 16 where it applies.  All variants
 * return identical results.  32 = class kernel (one check degree, bit degrees of a compiled range; auto picks it where it
 * applies and the local-edge kernel does not).  63 = HBM-resident min-sum kernel with whole check records in the workspace
 * (the form a code whose per-check data exceed the CU's LDS gets; ignored by the other kernels).  64 = the any-degree
 * kernel on any code (slow; a second implementation for cross-checks, also of the HBM-resident BP kernel). */
int bposd_set_bp_variant(bposd_handle *h, int32_t variant);

/*
 * Relay-BP (Mueller et al., 2025): a mode of the handle.  With it on, the BP stage of every decode call (host, device and
 * packed pointers, per-shot channels, observables, the DEM engine) runs min-sum as a chain of `legs` legs with a memory term
 * per bit.  The mode and its tables belong to one handle and its n bits: the window engine (bposd_window_*) runs every window
 * on the handle it was given for it, in relay mode where that handle is, so a windowed relay decode sets each window's handle
 * with the columns of its own faults (bp_osd_amd/window.py does).  The outputs, the OSD hand-off and the lane buffers are
 * those of every other BP kernel.  Per shot, with l0 the shot's prior LLRs:
 *   M = l0, dec = 0, every bit->check message = l0 of its bit, t = 0, found = 0.  An all-zero syndrome returns zeros,
 *   converged 1, 0 iterations (solutions 0, best_leg -1, weight 0).
 *   Leg r = 0 .. legs-1, g = gammas[r]: for r > 0 and leg_init == 0 the bit->check messages go back to l0 (leg_init == 1
 *   keeps them; M is always kept).  Up to leg_iters[r] times: t += 1; the min-sum check pass with the scaling factor of
 *   iteration t; the bit pass with  lam = (1 - g[j]) * l0[j] + g[j] * M[j]  (two products, one add, each rounded) in the
 *   place of the prior -- M[j] becomes the posterior, dec[j] = (M[j] <= 0).  If H dec == syndrome: found += 1,
 *   w = sum_j dec[j] * W[j] with W[j] = (int64) rint(clamp(l0[j], -32768, 32768) * 2^32); the solution replaces the best one
 *   if it is the first or w is strictly lower; the leg ends; after `stop_after` solutions the shot ends.
 *   Result: iterations = t.  found > 0: the bp, osd0 and osdw rows are the best solution, converged 1.  Otherwise the bp row
 *   is the last dec, converged 0, and with OSD enabled the shot goes to the OSD stage with M as its LLRs.  The LLR output
 *   is the final M.
 * legs = 1, gammas = 0, leg_iters = {max_iter}, stop_after = 1 is plain min-sum bit for bit (priors inside (0, 1)).
 *
 * bposd_set_relay copies gammas (float64 [legs][n]) and leg_iters (int32 [legs]) to the device after the calls in flight
 * have ended.  legs = 0 switches the mode off: the handle launches what it launched before.  BPOSD_ERR_INVALID (handle
 * unchanged) for legs < 0, a non-finite gamma, a leg of fewer than 1 iteration, stop_after < 1, leg_init other than 0 / 1
 * or NULL tables with legs > 0; BPOSD_ERR_UNSUPPORTED for product-sum or the serial schedule.
 *
 * bposd_relay_stats copies the per-shot words of the last call that ran on `lane` (-1: the lane of the last relay launch) to host arrays of B
 * entries, any of which may be NULL: solutions found, leg of the best one (-1: none), its weight.  It waits for that lane.
 * BPOSD_ERR_INVALID if that call did not run in relay mode or B is not its batch size.  With all three arrays NULL nothing
 * is copied and the return value is that call's batch size (>= 1).  A host-pointer call of several chunks leaves each
 * lane the words of its last chunk only.
 */
int bposd_set_relay(bposd_handle *h, int32_t legs, const double *gammas, const int32_t *leg_iters, int32_t stop_after,
                    int32_t leg_init);
int bposd_relay_stats(bposd_handle *h, int32_t lane, int32_t *solutions, int32_t *best_leg, int64_t *weight, int64_t B);

/*
 * BP+LSD (localized statistics decoding, Hillmann et al., 2024): a mode of the handle.  With it on, every decode
 * call (host, device and packed pointers, per-shot channels, observables, the DEM engine) runs lsd_kernel over the list of
 * shots BP left open, in front of the OSD kernel, which then decodes only the shots LSD did not solve.  Per listed shot,
 * with l its posterior LLRs as the OSD stage would get them:
 *   Bit a comes before bit b iff l[a] < l[b], ties by ascending bit index (sort_tie_policy 0) or descending (1): the order
 *   the OSD stage sorts columns in.  Every unsatisfied check starts as a cluster of its own without bits.  A cluster (checks
 *   C, bits V, every check of a bit of V is in C) is valid iff s[C] lies in the column span of H[C, V].
 *   A round: every cluster that is invalid at its start selects the first bit, in that order, among the bits that have a
 *   check in C and are in no cluster.  All selected bits join at once (two clusters may select the same bit), each with all
 *   its checks; clusters connected through a joined bit merge (valid ones may be swallowed), and the validity of every
 *   cluster that grew or merged is evaluated afresh.  Rounds repeat until every cluster is valid.
 *   Result: per cluster the solution of H[C, V] x = s[C] supported on the greedy column basis with V in the order above
 *   (OSD-0 restricted to the cluster); every other bit 0.  The result does not depend on the order clusters are visited in.
 *   status 0: solved -- the osdw and osd0 rows are that solution.  1: after some round a cluster held more than
 *   max_cluster_bits bits or max_cluster_checks checks.  2: at the start of a round an invalid cluster had no bit to select
 *   (the syndrome is outside the column space).  Shots of status 1 and 2 go to the OSD stage as BP left them; with
 *   osd_method off they keep BP's decisions.  rounds = rounds in which bits joined, clusters and max_bits = the number of
 *   clusters and the most bits in one of them when the shot ended.  Shots BP converged on: status -1, zeros.
 * The OSD stage's rows of the shots it decodes are those of a handle without the mode.  It is this project's synchronous
 * definition, not upstream ldpc's BpLsdDecoder, whose sequential growth order differs.
 *
 * Higher orders and growth for free bits (bposd_set_lsd_order; with its defaults -- BPOSD_LSD_0, order 0, min_free_bits 0,
 * grow_bits_limit 256 -- the definition is the one above).  Everything not named here stays as above.
 *   free = |V| - rank H[C, V]; the free columns of a cluster are the columns of V, in the order above, that are not in
 *   the greedy column basis.  A bit joins with all its checks, so growth and merges never lower free.
 *   A cluster is unfinished at the start of a round if it is invalid, or if it is valid, free < min_free_bits and
 *   |V| < grow_bits_limit.  Every unfinished cluster selects as invalid clusters do above.  An invalid cluster with nothing
 *   to select ends the shot with status 2; a valid unfinished cluster with nothing to select is finished and stays so
 *   until it changes through a merge.  Rounds repeat while some cluster selects.  The caps work as above: growth for free
 *   bits alone adds one bit at a time and stops at grow_bits_limit, but merges, and the checks joining bits bring, can
 *   still overflow a cap (status 1).
 *   On a solved shot the osd0 row is, per final cluster, the solution on the greedy column basis (the row above, on the
 *   possibly larger clusters); the osdw row is, per final cluster, the lightest candidate of a sweep over the cluster's
 *   reduced system.  With kp free columns and w' = min(order, kp), the baseline is the osd0 solution; BPOSD_LSD_CS tries
 *   the kp single free columns in column order, then the pairs (a < b < w') with a outer and b inner; BPOSD_LSD_E tries
 *   the patterns 1 .. 2^w' - 1, bit b of a pattern standing for free column b (for free column w' - 1 - b if the handle's
 *   osd_e_bit_order is 1).  A candidate sets the free columns of its pattern to 1, every other free column to 0, and
 *   solves the basis bits from the reduced rows.  Its weight is the OSD stage's weight for that shot restricted to V: the
 *   number of set bits where the OSD kernels count bits (a uniform channel 0 < p < 1, or weight_fn = 1), otherwise the
 *   fp64 sum, started at 0.0, of log(1/p_j) over the set bits of V in ascending bit index, p being the channel the OSD
 *   kernel would use for that shot (the handle's, the two-valued per-shot choice, or the shot's own row).  A strictly
 *   lighter candidate replaces the best, so the first one found wins ties (oracle/bposd_oracle.c:488-523 inside a
 *   cluster): a cluster that holds every bit of the matrix gives the osd_cs / osd_e rows.
 *   Two more words per listed shot: max_free = the most free columns in one final cluster, improved = 1 iff the osdw row
 *   differs from the osd0 row; both are 0 unless status is 0.
 *
 * bposd_set_lsd(on = 0) switches the mode off: the handle launches what it did before and allocates nothing more for the
 * mode; what the mode has allocated (H by column, each lane's second list with its LLR rows, the four words per shot) stays
 * with the handle until it is destroyed, ready for the next switch-on.  A handle that never had the mode on holds none of
 * it.  BPOSD_ERR_INVALID
 * (handle unchanged) for a cap outside [1, 256], the kernel's ceilings (4 rows per lane of a 64-lane wave, 4 words per
 * row); BPOSD_ERR_UNSUPPORTED while relay mode is on (and bposd_set_relay while this mode is on), or if the cluster state of
 * the handle's shape does not fit one CU's LDS (no shape a handle is created for: 4 bytes + 1 bit per check, 2 bits per
 * bit and 12 864 bytes for one elimination -- 88 640 bytes at 16384 x 32767).
 *
 * bposd_lsd_stats: as bposd_relay_stats, for the four words per shot of the last call that ran on `lane` (-1: the lane of
 * the last LSD launch); any array may be NULL, all NULL returns that call's batch size.
 *
 * bposd_set_lsd_order holds method (BPOSD_LSD_0 / _CS / _E), order (0 with BPOSD_LSD_0; 1..64 with _CS; 1..10 with _E),
 * min_free_bits (0..64) and grow_bits_limit (1..256) on the handle; they take effect while LSD mode is on, in the calls
 * that follow, and survive switching the mode off and on.  A fresh handle has the defaults.  A sweep or min_free_bits > 0
 * selects the second instance of lsd_kernel, which holds a second row bitmap and the sweep's tables in LDS (1 bit per bit
 * and 1 536 bytes more) and six words per shot; otherwise the LSD-0 instance runs as before.  BPOSD_ERR_INVALID (handle
 * unchanged) names the value out of range; BPOSD_ERR_UNSUPPORTED (handle unchanged) if the mode is on and the second
 * instance's state does not fit one CU's LDS.  bposd_set_lsd checks the LDS of the instance in force.
 *
 * bposd_lsd_order_stats: as bposd_lsd_stats, for max_free and improved; zeros after a call of the LSD-0 instance.
 */
enum { BPOSD_LSD_0 = 0, BPOSD_LSD_CS = 1, BPOSD_LSD_E = 2 };
int bposd_set_lsd(bposd_handle *h, int32_t on, int32_t max_cluster_bits, int32_t max_cluster_checks);
int bposd_lsd_stats(bposd_handle *h, int32_t lane, int32_t *status, int32_t *rounds, int32_t *clusters, int32_t *max_bits,
                    int64_t B);
int bposd_set_lsd_order(bposd_handle *h, int32_t method, int32_t order, int32_t min_free_bits, int32_t grow_bits_limit);
int bposd_lsd_order_stats(bposd_handle *h, int32_t lane, int32_t *max_free, int32_t *improved, int64_t B);

/*
 * Monte-Carlo engine: the device-resident form of the reference's harness loop
 * (/root/reference/src/bposd/css_decode_sim.py:174-365, 465-498).  One bposd_mc_run is one batch of shots:
 * sample the errors -> both syndromes -> the two decodes -> logical checks of the bp / osd0 / osdw outputs -> seven
 * integers.  The handle owns every device buffer of a batch, so a device-resident simulation needs no torch (or any
 * other tensor library); bp_osd_amd/sim.py drives it as css_decode_sim(engine="native").
 *
 * Random stream (defined by this project, the same on host and device, independent of the batch size): Philox4x32-10.
 * For shot s (global, 64 bit), qubit i and the 64-bit seed:
 *   counter = (s & 0xffffffff, s >> 32, i >> 1, 0), key = (seed & 0xffffffff, seed >> 32), (o0, o1, o2, o3) = philox(counter, key)
 *   (a, b) = (o0 >> 5, o1 >> 6) for even i, (o2 >> 5, o3 >> 6) for odd i;  u = (a * 2^26 + b) * 2^-53
 *   Z if u < pz, X if pz <= u < pz + px, Y if pz + px <= u < px + py + pz; error_z = Z | Y, error_x = X | Y
 * (the thresholds in fp64, in that operation order: css_decode_sim.py:476-490).  Shot s of a run is row s - first_shot.
 */
typedef struct bposd_mc bposd_mc;

enum { BPOSD_MC_UPDATE_NONE = 0, BPOSD_MC_UPDATE_X_TO_Z = 1, BPOSD_MC_UPDATE_Z_TO_X = 2 };

typedef struct {
    int32_t device;          /* HIP device ordinal; both decoders must live there                              */
    int32_t channel_update;  /* BPOSD_MC_UPDATE_*: css_decode_sim.py:207-248                                     */
    uint64_t seed;           /* key of the random stream                                                       */
    int64_t capacity;        /* largest batch a run may ask for: every per-batch buffer is allocated for it     */
} bposd_mc_config;

/* What bposd_mc_fetch copies out of the last batch (B rows each). */
enum {
    BPOSD_MC_ERROR_X = 0,           /* uint64[B][ceil(n/64)]: packed rows, the layout of bposd_decode_batch_packed    */
    BPOSD_MC_ERROR_Z = 1,
    BPOSD_MC_SYNDROME_X = 2,        /* uint8[B][mz]: hz . error_x                                                   */
    BPOSD_MC_SYNDROME_Z = 3,        /* uint8[B][mx]: hx . error_z                                                   */
    BPOSD_MC_FLAGS = 4,             /* uint8[B]: bit 0 / 1 bp failed the X- / Z-logical check, 2 / 3 osd0, 4 / 5 osdw */
    BPOSD_MC_SYNDROME_X_PACKED = 5, /* uint64[B][ceil(mz/64)]                                                       */
    BPOSD_MC_SYNDROME_Z_PACKED = 6  /* uint64[B][ceil(mx/64)]                                                       */
};

/*
 * dec_x decodes hz . error_x, dec_z decodes hx . error_z (css_decode_sim.py:444-463); they stay the caller's and must
 * outlive the engine.  hx [mx x n] and hz [mz x n] as CSR; lx, lz as k packed rows of ceil(n/64) words; probs_* [n] the
 * per-qubit probabilities of X, Y and Z errors.  With a channel update, the decoder that runs second must already hold
 * the probabilities for "the first decoder's osdw bit is 0" (bposd_update_channel_probs), and alt_probs [n] are those for
 * "bit is 1" (css_decode_sim.py:217-227, 236-246); alt_probs may be NULL without a channel update.  Everything is copied.
 */
int bposd_mc_create(const bposd_mc_config *cfg, bposd_handle *dec_x, bposd_handle *dec_z, const int32_t *hx_indptr,
                    const int32_t *hx_indices, int32_t mx, const int32_t *hz_indptr, const int32_t *hz_indices, int32_t mz,
                    int32_t n, const uint64_t *lx_words, const uint64_t *lz_words, int32_t k, const double *probs_x,
                    const double *probs_y, const double *probs_z, const double *alt_probs, bposd_mc **out);

/*
 * One batch: shots first_shot .. first_shot + B - 1 (B <= capacity).  Returns with the counters on the host:
 *   [0] bp_converge_count_x  [1] bp_converge_count_z  [2] bp_success_count (both converged, no logical failure)
 *   [3] osd0_success_count   [4] osdw_success_count
 *   [5], [6] smallest weight of a failing residual of osd0 / osdw (INT32_MAX when nothing failed); the weight is that of
 *   residual_x where the X-logical check failed, else of residual_z (css_decode_sim.py:257-272)
 * Without a channel update the two decodes run side by side on their handles' lanes, otherwise the second one takes the
 * first one's osdw rows through the per-shot channel of bposd_decode_batch_select_device.  The engine's stream and the
 * lanes are ordered by events; the one host wait of a batch is the one for the counters.
 */
int bposd_mc_run(bposd_mc *mc, uint64_t first_shot, int64_t B, int64_t counters[7]);

/* Copy one item (BPOSD_MC_ERROR_X ...) of the last batch to host memory; bytes must be that item's size for the last B. */
int bposd_mc_fetch(bposd_mc *mc, int32_t what, void *host_dst, size_t bytes);

/* Device memory the engine holds (the sum of its own allocations; the decoders' workspaces are theirs). */
int64_t bposd_mc_device_bytes(bposd_mc *mc);

/* Message for the last error on this engine (mc == NULL: the last bposd_mc_create failure). */
const char *bposd_mc_last_error(bposd_mc *mc);

void bposd_mc_destroy(bposd_mc *mc);

/*
 * Detector-error-model Monte-Carlo engine: the second engine, for circuit-level and phenomenological models.  A model is
 * a check matrix H (M detectors x N fault mechanisms), an observable matrix L (k x N) and one prior per mechanism; nothing
 * of it is CSS-shaped.  One bposd_dem_run is one batch of shots: sample the faults f -> detector row H . f and true
 * observable row L . f -> one decode straight to observables (bposd_decode_batch_observables_device) -> compare -> five
 * integers.  The engine owns every device buffer of a batch and needs no torch; bp_osd_amd/dem.py drives it as
 * dem_decode_sim(engine="native").  (No counterpart in the reference: its harness is the code-capacity CSS loop above.)
 *
 * Random stream: the one defined above ("Random stream"), with the fault index in the place of the qubit index.  Fault i
 * of global shot s fires iff u(s, i) < priors[i]: counter (s lo, s hi, i >> 1, 0), key = seed, (o0, o1) serve even i and
 * (o2, o3) odd i, u = uniform53; the compare is in fp64 against priors[i] as given (0 never fires, 1 always does).
 * Host restatement: sim.philox_uniforms(seed, first_shot, B, N) < priors.  Shot s of a run is row s - first_shot.
 *
 * The sampler scatters: a fault that fired walks its column of H stacked on L and flips one bit per entry of the shot's
 * row in LDS (XOR commutes: the row is bit-exact whatever the arrival order).  bposd_dem_tables builds that CSC.
 */
typedef struct bposd_dem bposd_dem;

typedef struct {
    int32_t device;    /* HIP device ordinal; the decoder must live there                                     */
    uint64_t seed;     /* key of the random stream                                                            */
    int64_t capacity;  /* largest batch a run may ask for: every per-batch buffer is allocated for it         */
} bposd_dem_config;

/* What bposd_dem_fetch copies out of the last batch (B rows each, but for the last item). */
enum {
    BPOSD_DEM_FAULTS = 0,      /* uint64[B][ceil(N/64)]: packed rows, the layout of bposd_decode_batch_packed         */
    BPOSD_DEM_DETECTORS = 1,   /* uint64[B][ceil(M/64)]: H . faults                                                   */
    BPOSD_DEM_OBSERVABLES = 2, /* uint64[B][ceil(k/64)]: L . faults, the true observables                             */
    BPOSD_DEM_OBS_BP = 3,      /* uint64[B][ceil(k/64)]: L . correction of the bp / osd0 / osdw output, as decoded    */
    BPOSD_DEM_OBS_OSD0 = 4,
    BPOSD_DEM_OBS_OSDW = 5,
    BPOSD_DEM_FLAGS = 6,       /* uint8[B]: bit 0 bp wrong, bit 1 osd0 wrong, bit 2 osdw wrong, bit 3 no detector fired */
    BPOSD_DEM_CONVERGED = 7,   /* uint8[B]                                                                            */
    BPOSD_DEM_ITERS = 8,       /* int32[B]                                                                            */
    BPOSD_DEM_OBS_FAIL = 9,    /* int32[k]: osdw failures per observable in this batch                                */
    BPOSD_DEM_LOGW = 10,       /* int64[B]: the shot's log-weight in units of 2^-32 (weighted sampling only, see below) */
    /* the harvest of the last batch (bposd_dem_set_harvest below): F failing shots, K = max_rows */
    BPOSD_DEM_FAIL_ROWS = 11,     /* int32[F]: the failing rows, ascending                                            */
    BPOSD_DEM_FAIL_WEIGHT = 12,   /* int32[F]: weight of the residual, aligned with FAIL_ROWS                         */
    BPOSD_DEM_FAIL_RESIDUAL = 13, /* uint64[min(F, K)][ceil(N/64)]: faults XOR correction of the first failing rows   */
    BPOSD_DEM_FAIL_FAULTS = 14,   /* uint64[min(F, K)][ceil(N/64)]: their fault rows                                  */
    BPOSD_DEM_MIN_RESIDUAL = 15   /* uint64[ceil(N/64)]: the residual of the lightest failing row, zeros when F = 0   */
};

/*
 * CSR of H (h_indptr[M+1]) and of L (l_indptr[k+1]) -> the stacked CSC the sampler reads: col_ptr[N+1], and col_bits[nnz(H)
 * + nnz(L)] holding, per fault and ascending, the bits it flips -- detector r is bit r, observable j is bit
 * 64 * ceil(M/64) + j, so that the detector words and the observable words of a row are contiguous ranges of one array.
 * Host only: no handle, no device.  BPOSD_ERR_INVALID (text: bposd_last_error(NULL)) for a column outside [0, N), columns
 * that do not ascend strictly within a row, k outside 1 .. 4096, M < 1 or N < 1; nothing is written then.  Columns without
 * an entry are legal, and so are columns that touch observables only.
 */
int bposd_dem_tables(const int32_t *h_indptr, const int32_t *h_indices, int32_t M, const int32_t *l_indptr,
                     const int32_t *l_indices, int32_t k, int32_t N, int32_t *col_ptr, int32_t *col_bits);

/*
 * priors[N]: each in [0, 1], a NaN is refused (the message names the fault).  With a decoder: dec's (m, n) must be (M, N)
 * and it must live on cfg->device; THE ENGINE SETS THE DECODER'S OBSERVABLE TABLE -- it builds the table of L and installs
 * it with bposd_set_observables(dec, ...), so that the L that scores and the L the decoder multiplies by cannot differ
 * (a run after someone replaced that table by one of another k is refused).  The decoder's channel stays whatever its
 * owner gave it; the Python layer passes the priors to both.  dec == NULL makes a sample-only engine, on which
 * bposd_dem_run returns BPOSD_ERR_INVALID.  Everything is copied; the decoder stays the caller's and must outlive the
 * engine; the table is installed last, so a create that fails leaves the decoder as it was.  BPOSD_ERR_UNSUPPORTED for a model whose row of M + k bits does not fit the sampler's LDS (two rows in 64 KB).
 */
int bposd_dem_create(const bposd_dem_config *cfg, bposd_handle *dec, const int32_t *h_indptr, const int32_t *h_indices,
                     int32_t M, const int32_t *l_indptr, const int32_t *l_indices, int32_t k, int32_t N,
                     const double *priors, bposd_dem **out);

/*
 * Importance sampling: draw the faults from a harsher row q = sample_priors[N] while the decoder keeps the model's priors p
 * as its channel, and leave a per-shot log-likelihood ratio.  Fault i of global shot s then fires iff u(s, i) < q[i] -- the
 * same stream, the same counter -- and item BPOSD_DEM_LOGW holds, per shot, the sum of incr[i] over the faults that fired:
 * an integer sum, so it does not depend on the order in which lanes and atomics arrive and is bit-exact on every device,
 * batch size and host restatement (faults.astype(int64) @ incr).  The caller chooses incr; for the likelihood ratio
 * w = prod_i (p_i/q_i)^f_i ((1-p_i)/(1-q_i))^(1-f_i) of a shot with fault row f it is
 *     incr[i] = round(a_i * 2^32),  a_i = log(p_i / q_i) - log((1 - p_i) / (1 - q_i))   (0 where p_i == q_i),
 *     c0 = sum_i log((1 - p_i) / (1 - q_i)),                  w = exp(c0 + logw / 2^32),
 * with q_i == 0 only where p_i == 0 and q_i == 1 only where p_i == 1 (bp_osd_amd.dem.importance_table computes exactly
 * this and refuses the rest).  The rounding moves a weight by at most 2^-33 relative per fired fault.
 *
 * Both arrays are copied.  Every q[i] must be in [0, 1] (a NaN is refused, the message names the fault) and the sum of
 * |incr[i]| must be below 2^62, so that no shot can overflow; NULL for one pointer only is refused; a refusal leaves the
 * engine in the mode it was in.  NULL, NULL switches back to plain sampling.  Works on sample-only engines too.  The first
 * call allocates the two tables and int64[capacity] (counted in bposd_dem_device_bytes).  The five counters of
 * bposd_dem_run stay unweighted counts of the shots as sampled.  A sample-only engine handed to bposd_window_run draws in
 * the mode it is in; that engine's own results know nothing of weights.
 */
int bposd_dem_set_sampling(bposd_dem *dem, const double *sample_priors, const int64_t *incr);

/*
 * Fault sets of a fixed weight: a shot is then not a Bernoulli row but a set of exactly `weight` = w of the n mechanisms of
 * a support -- every set of a stratum in turn (a proof that the decoder corrects all of them, or the list of those it does
 * not), or sets drawn uniformly (stratified sampling: LER = sum_w P(|f| = w, fail)).  support[n_support] is an ascending
 * list of distinct fault indices, NULL stands for all N (n_support is then ignored); position c of a set is fault
 * support[c]; 0 <= w <= min(n, 64).
 *
 *   BPOSD_DEM_SUBSET_ENUMERATE: global shot s is the set of rank s in colexicographic order (the combinatorial number
 *     system): from r = s, for j = w .. 1, c_j = the largest c with C(c, j) <= r, r -= C(c_j, j); the set is
 *     {c_1 < ... < c_w}.  Ranks 0 .. 4 of n = 7, w = 3 are (0,1,2), (0,1,3), (0,2,3), (1,2,3), (0,1,4); the last is (4,5,6);
 *     w = 0 is the one empty set.  C(n, w) must be below 2^63, and a batch with first_shot + B > C(n, w) is refused.
 *   BPOSD_DEM_SUBSET_RANDOM: Floyd's algorithm on the random stream.  For step i = 0 .. w - 1 with j = n - w + i: counter
 *     (s lo, s hi, i >> 1, 1), key = seed -- the fourth counter word 1 keeps these draws apart from the Bernoulli stream,
 *     which uses 0 -- u = o[2 (i & 1)] | o[2 (i & 1) + 1] << 32, t = (u * (j + 1)) >> 64; the step takes j if t is already
 *     in the set, else t.  Every w-subset is equally likely up to the multiply-shift bias: t takes each of its j + 1 values
 *     with probability 1 / (j + 1) +- 2^-64, a relative bias below (j + 1) / 2^64 < 2^-49 per step (j < 2^15).  The draw
 *     does not depend on the batch size or the device.
 *   BPOSD_DEM_SUBSET_OFF: back to Bernoulli rows (weight, support and incr are ignored); a batch then launches and allocates
 *     what it did before.
 *
 * Items 0-2 of a shot are those of the Bernoulli sampler for that fault row (packed, padding zero; H . f; L . f), and
 * everything behind the sampler -- decode, scorer, harvest -- runs unchanged.  With incr[N] (may be NULL) item
 * BPOSD_DEM_LOGW holds the integer sum of incr over the set; the item is valid if and only if incr was given.  For the
 * probability of a set under the priors, incr[i] = round(log(p_i / (1 - p_i)) * 2^32) and c0 = sum over the support of
 * log(1 - p_i) give P(set) = exp(c0 + logw / 2^32) (bp_osd_amd.dem.subset_table).
 *
 * The arrays are copied (counted in bposd_dem_device_bytes: C(c, j) for j = 1 .. w, c = 0 .. n in enumerate mode, the
 * increments, the support, and int64[capacity] with the first increment table).  Works on sample-only engines; one in a
 * subset mode that is handed to bposd_window_run draws that way (that engine's results know nothing of strata).
 * BPOSD_ERR_INVALID, with a message that names the culprit and the engine left as it was, for: a mode that is none of
 * the three; a weight outside [0, min(n, 64)]; a support that does not ascend strictly or leaves [0, N); C(n, w) >= 2^63 in
 * enumerate mode; w * |incr[i]| >= 2^62 for a fault of the support; weighted sampling switched on (and
 * bposd_dem_set_sampling with a table is refused while a subset mode is on): switch one off first.  BPOSD_ERR_UNSUPPORTED
 * where four rows of M + k + N bits do not fit the sampler's LDS (64 KB).
 */
#define BPOSD_DEM_SUBSET_OFF 0
#define BPOSD_DEM_SUBSET_ENUMERATE 1
#define BPOSD_DEM_SUBSET_RANDOM 2
int bposd_dem_set_subset(bposd_dem *dem, int32_t mode, int32_t weight, const int32_t *support, int32_t n_support,
                         const int64_t *incr);

/* The sampler alone: shots first_shot .. first_shot + B - 1 (1 <= B <= capacity); waits for the kernel.  Items 0-2 of
 * bposd_dem_fetch hold the batch afterwards (and item 10 while weighted sampling is on, or a subset mode with increments). */
int bposd_dem_sample(bposd_dem *dem, uint64_t first_shot, int64_t B);

/*
 * One batch: sample on the engine's stream, decode on the decoder's next lane (ordered by events), score on the engine's
 * stream.  Returns with the counters on the host -- the one host wait of a batch:
 *   [0] bp converged   [1] bp success (converged AND observables equal the true ones)   [2] osd0 success
 *   [3] osdw success   [4] shots in which no detector fired
 * B outside [1, capacity] is BPOSD_ERR_INVALID.  Items 0-9 of bposd_dem_fetch hold the batch afterwards (and item 10 while
 * weighted sampling is on).
 */
int bposd_dem_run(bposd_dem *dem, uint64_t first_shot, int64_t B, int64_t counters[5]);

/*
 * Harvest of failing shots: with max_rows = K >= 1 every bposd_dem_run also keeps, on the device and behind its scorer, the
 * shots whose osdw observables are wrong (flag bit 2).  For such a row b with fault row f_b and osdw correction c_b the
 * residual r_b = f_b XOR c_b has H r_b = 0 (osdw reproduces a consistent syndrome) and L r_b != 0: an undetected logical
 * fault set, whose weight w_b = popcount(r_b) bounds the model's fault distance from above.  Per batch:
 *     items 11 .. 15 of bposd_dem_fetch (above), and bposd_dem_harvest_info: out[0] = F, the number of failing shots,
 *     out[1] = the least w_b over ALL of them, out[2] = the LOWEST row that has it; -1, -1 when F = 0.
 * Rows are listed in ascending order by prefix sums and a tie in weight goes to the lowest row: nothing depends on the order
 * in which waves arrive, and the host restatement (bp_osd_amd._dem_base.harvest_batch) gives the same bits.  bp and osd0
 * rows are not harvested (a bp row that did not converge does not reproduce the syndrome).
 *
 * Three small kernels (csrc/harvest_kernels.hip.h) run on the engine's stream between the scorer and the counters'
 * download; the triple comes down with the counters, so a batch keeps its one host wait.  The correction rows are read
 * where the decode left them, in the buffers of the decoder lane it ran on: they stay valid because bposd_dem_run ends in
 * its host wait before anything else can be queued on that lane.
 *
 * max_rows = 0 switches off (the default; the block stays allocated): then a batch launches and allocates nothing more
 * than it did before.  Negative: BPOSD_ERR_INVALID; so is a sample-only engine.  A refusal leaves the engine as it was.
 * The first call with K >= 1 (and a later call with a larger K, which replaces the block) allocates one block of
 *     8 capacity + (2 K + 1) * 8 ceil(N/64) + 256   bytes
 * -- list and weights, K residual and K fault rows, the lightest residual (it need not be among the first K, so it has a
 * row of its own), 256 bytes of kernel state (the running minimum and the count between the launches) -- counted in
 * bposd_dem_device_bytes.  bposd_dem_harvest_info is a host copy (no device call) and, like items 11 .. 15, is refused
 * unless the last batch ran with the harvest on.
 */
int bposd_dem_set_harvest(bposd_dem *dem, int64_t max_rows);
int bposd_dem_harvest_info(bposd_dem *dem, int64_t out[3]);

/*
 * Per-fault sums over selected shots of the last batch -- a reduced fetch: with f_b the fault row of shot b (item
 * BPOSD_DEM_FAULTS), b_0 < b_1 < ... the selected rows and mult[s] a 32-bit multiplier of the s-th of them,
 *     counts[i] = sum_s f_{b_s}[i]        sums[i] = sum_s mult[s] f_{b_s}[i]        i = 0 .. N - 1
 * as 64-bit integers (no sum can reach 2^63: mult < 2^32 and fewer than 2^31 rows).  With the likelihood ratios of the
 * failing shots as multipliers (bp_osd_amd.dem.weight_multipliers) sums[i] / sum_s mult[s] is the cross-entropy update of
 * fault i's sampling probability (bp_osd_amd.dem.fit_sample_priors); counts alone say which mechanisms the failures are
 * made of.  The rows stay on the device: 4 n_mult bytes go up and 8 N (mult == NULL) or 16 N come down, where fetching the
 * rows would move 8 ceil(N/64) bytes per shot.
 *   BPOSD_DEM_SELECT_ALL: every shot of the last batch, after bposd_dem_run or bposd_dem_sample; mult is [B].
 *   BPOSD_DEM_SELECT_FAILING: the failing shots the harvest listed in the last batch (BPOSD_DEM_FAIL_ROWS), read where the
 *     harvest left the list; mult is [F], aligned with that item.  Needs a batch that ran with the harvest on.
 * One kernel (csrc/fault_sums_kernel.hip.h) on the engine's stream; the call waits.  Integer adds only: the result does not
 * depend on the order of arrival, and the host restatement (bp_osd_amd._dem_base.fault_sums_batch) gives the same bits.  A
 * row with multiplier 0 still counts in counts.  mult and sums go together (both, or NULL for both: counts only); n_mult is
 * ignored when mult is NULL.
 *
 * BPOSD_ERR_INVALID, with the engine left as it was: a select that is neither of the two, no batch yet, FAILING without a
 * harvested batch, n_mult different from B (ALL) or F (FAILING), counts == NULL, one of mult and sums without the other.
 * The first call that passes these checks allocates one block of  16 N + 4 capacity  bytes (the two arrays and the
 * multipliers), counted in bposd_dem_device_bytes; an engine that never calls this launches, allocates and downloads what it
 * did before.  bposd_dem_run is not involved.  (The sliding-window engine has no such call: its run knows nothing of
 * weights.  The rows of its sampler are a sample-only bposd_dem's, on which BPOSD_DEM_SELECT_ALL works.)
 */
#define BPOSD_DEM_SELECT_ALL 0     /* every shot of the last batch; mult is [B]                                        */
#define BPOSD_DEM_SELECT_FAILING 1 /* the harvest's failing rows of the last batch; mult is [F], aligned with FAIL_ROWS */
int bposd_dem_fault_sums(bposd_dem *dem, int32_t select, const uint32_t *mult, int64_t n_mult, uint64_t *counts,
                         uint64_t *sums);

/* Copy one item (BPOSD_DEM_FAULTS ...) of the last batch to host memory; bytes must be that item's size for the last B
 * (for items 11 .. 14: for the last batch's number of failing shots -- 0 bytes is legal and copies nothing).
 * After bposd_dem_sample only items 0-2 are there.  BPOSD_DEM_OBS_FAIL came down with the counters: no device call.
 * BPOSD_DEM_LOGW needs a batch sampled while weighted sampling is on, or a subset mode that was given increments:
 * BPOSD_ERR_INVALID otherwise. */
int bposd_dem_fetch(bposd_dem *dem, int32_t what, void *host_dst, size_t bytes);

/* Device memory the engine holds (the sum of its own allocations; the decoder's workspaces are its own). */
int64_t bposd_dem_device_bytes(bposd_dem *dem);

/* Message for the last error on this engine (dem == NULL: the last bposd_dem_create / bposd_dem_tables failure). */
const char *bposd_dem_last_error(bposd_dem *dem);

void bposd_dem_destroy(bposd_dem *dem);

/*
 * Sliding-window engine: a detector error model decoded window by window along time, every window on a decoder of its own,
 * all of it on the device.  Decoding a model as one matrix meets the size limits above after a few rounds and costs more
 * per round the longer the experiment is; here the cost per round is constant.  bp_osd_amd/window.py builds the windows
 * (window_plan) and drives the engine as WindowedDemDecoder and windowed_dem_decode_sim(engine="native"); DESIGN.md 4.12
 * has the definition.  (No counterpart in the reference.)
 *
 * The model is H (M x N), L (k x N); window w is a list D_w of detectors and a list F_w of faults, both ascending, a commit
 * flag per entry of F_w, and a decoder for H[D_w][:, F_w].  Per shot, with r = the detector row, obs = 0, corr = 0, and
 * for w = 0 .. nwin - 1 in order:
 *     s = r[D_w]  ->  osdw row c of decs[w]  ->  for every j with commit flag 1 and c_j = 1:
 *         r ^= H[:, F_w[j]] (the whole column),  obs ^= L[:, F_w[j]],  corr[F_w[j]] = 1.
 * Outputs per shot: obs (ceil(k/64) words), corr (ceil(N/64) words), the final r (ceil(M/64) words; zero where every window
 * has full row rank, which window_plan checks), "BP converged in every window" and the windows' iteration counts summed.
 *
 * Between two decodes runs one window_step_kernel (csrc/window_kernels.hip.h): it commits window w - 1 and gathers the
 * syndrome of window w, staging in LDS only the words of the detector row that the step can touch.  nwin + 1 launches per
 * batch; the first only gathers, the last only commits.  Window w's decode is the plain device-pointer call of decs[w]
 * (packed rows where that decoder's kernels take them, byte rows otherwise) on its next lane, ordered against the engine's
 * stream by events.  The windows of a batch run one after another; the batch is the parallelism.
 */
typedef struct bposd_window bposd_window;

typedef struct {
    int32_t device;    /* HIP device ordinal; every decoder must live there                                   */
    int64_t capacity;  /* largest batch of one device call: every per-batch buffer is allocated for it        */
} bposd_window_config;

/* What bposd_window_fetch copies out of the last bposd_window_run (B rows each, but for the last item). */
enum {
    BPOSD_WINDOW_OBS = 0,         /* uint64[B][ceil(k/64)]: L . correction                                            */
    BPOSD_WINDOW_OBSERVABLES = 1, /* uint64[B][ceil(k/64)]: L . faults, the true observables (copied from the sampler) */
    BPOSD_WINDOW_CORRECTION = 2,  /* uint64[B][ceil(N/64)]                                                            */
    BPOSD_WINDOW_RESIDUAL = 3,    /* uint64[B][ceil(M/64)]: the detector row behind the last window                   */
    BPOSD_WINDOW_FLAGS = 4,       /* uint8[B]: bit 0 observables wrong, bit 1 residual not zero, bit 3 no detector fired */
    BPOSD_WINDOW_CONVERGED = 5,   /* uint8[B]: BP converged in every window                                           */
    BPOSD_WINDOW_ITERS = 6,       /* int32[B]: BP iterations summed over the windows                                  */
    BPOSD_WINDOW_OBS_FAIL = 7,    /* int32[k]: failures per observable in this batch                                  */
    /* the harvest of the last batch (bposd_window_set_harvest below), as items 11 .. 15 of bposd_dem_fetch */
    BPOSD_WINDOW_FAIL_ROWS = 8,
    BPOSD_WINDOW_FAIL_WEIGHT = 9,
    BPOSD_WINDOW_FAIL_RESIDUAL = 10,
    BPOSD_WINDOW_FAIL_FAULTS = 11,
    BPOSD_WINDOW_MIN_RESIDUAL = 12
};

/*
 * H and L as CSR (columns strictly ascending within a row, as bposd_dem_tables takes them).  Window w holds detectors
 * win_det[win_det_ptr[w] .. win_det_ptr[w+1]) and faults win_fault[win_fault_ptr[w] .. win_fault_ptr[w+1]), and
 * win_commit has one byte (0 / 1) per entry of win_fault.  BPOSD_ERR_INVALID, with the window named in the text
 * (bposd_window_last_error(NULL)), for an empty list, an index out of range or lists that do not ascend strictly, a fault
 * committed by two windows, a decoder that is NULL, lives on another device or whose (m, n) is not (|D_w|, |F_w|), or whose
 * matrix is not H[D_w][:, F_w].  BPOSD_ERR_UNSUPPORTED for a step whose staged words -- detector words in range, ceil(k/64)
 * observable words, the correction words its commit list touches -- exceed 64 KB of LDS.  Everything is copied.  The
 * engine touches neither the decoders' channels nor their observable tables; decoders may be shared between windows and
 * between engines, stay the caller's and must outlive the engine.
 *
 * Device memory (bposd_window_device_bytes; every block is at least 256 bytes), with cap = capacity, dw = ceil(M/64),
 * ow = ceil(k/64), fw = ceil(N/64), nc = commit entries over all windows, ncw = correction words over all steps,
 * synd / dec = the largest syndrome / decoded row of a window in its decoder's form (packed: 8 ceil(./64) bytes; else one
 * byte per entry):
 *     tables   4 (N + 1) + 4 (nnz(H) + nnz(L))  col_ptr, col_bits;   3 * 4 nc  commit pos / fault / slot;   4 ncw;   4 sum |D_w|
 *     batch    8 cap (dw + 2 ow + fw)    running detector rows, observables, true observables, correction
 *              cap (synd + dec)          the current window's syndrome and decoded rows
 *              cap (1 + 4 + 1 + 4 + 1)   converged and iterations (all windows; current window), flags
 *              4 * 8 + 4 k               counters, obs_fail
 */
int bposd_window_create(const bposd_window_config *cfg, int32_t M, int32_t N, int32_t k, const int32_t *h_indptr,
                        const int32_t *h_indices, const int32_t *l_indptr, const int32_t *l_indices, int32_t nwin,
                        bposd_handle *const *decs, const int32_t *win_det_ptr, const int32_t *win_det,
                        const int32_t *win_fault_ptr, const int32_t *win_fault, const uint8_t *win_commit,
                        bposd_window **out);

/* Decode B (1 <= B <= capacity) packed detector rows, every pointer a DEVICE pointer on the engine's device:
 * d_detector_words [B][ceil(M/64)] in (padding bits zero; not written), d_obs_words [B][ceil(k/64)] out; optional (NULL:
 * not wanted) d_correction_words [B][ceil(N/64)], d_residual_words [B][ceil(M/64)], d_conv uint8[B], d_iters int32[B].
 * Asynchronous on the engine's own stream, which is not ordered against the caller's streams: the inputs must be complete
 * at the call, and bposd_window_synchronize comes before the outputs are read or the next call is made with the same
 * buffers.  Calls on one engine run one after another. */
int bposd_window_decode_device(bposd_window *win, const uint64_t *d_detector_words, int64_t B, uint64_t *d_obs_words,
                               uint64_t *d_correction_words, uint64_t *d_residual_words, uint8_t *d_conv, int32_t *d_iters);
int bposd_window_synchronize(bposd_window *win);

/* The same with HOST pointers and any B >= 0: runs in chunks of `capacity`, synchronous. */
int bposd_window_decode(bposd_window *win, const uint64_t *detector_words, int64_t B, uint64_t *obs_words,
                        uint64_t *correction_words, uint64_t *residual_words, uint8_t *conv, int32_t *iters);

/*
 * One Monte-Carlo batch: `sampler` -- a sample-only bposd_dem (dec == NULL) of the same M, N, k and device, which holds the
 * priors and the seed -- samples shots first_shot .. first_shot + B - 1 on its stream, the windows run here, the scorer
 * compares, and the call returns with the counters on the host: the one host wait of a batch.
 *   [0] BP converged in every window   [1] success (observables equal the true ones)
 *   [2] residual not zero              [3] shots in which no detector fired
 * Afterwards bposd_window_fetch holds the batch, and items 0-2 of bposd_dem_fetch(sampler, ...) its faults, detectors and
 * true observables.
 */
int bposd_window_run(bposd_window *win, bposd_dem *sampler, uint64_t first_shot, int64_t B, int64_t counters[4]);

/*
 * Harvest of failing shots, as bposd_dem_set_harvest / bposd_dem_harvest_info define it, with the engine's own rows: a shot
 * fails when its observables are wrong (flag bit 0) and its final residual detector row is zero (bit 1 clear), c_b is the
 * committed correction row and f_b the sampler's fault row; H (f_b XOR c_b) = 0 is the zero residual.  Same items (8 .. 12),
 * same block and byte count, same rules for 0, a negative K and the refusals; only bposd_window_run harvests.
 */
int bposd_window_set_harvest(bposd_window *win, int64_t max_rows);
int bposd_window_harvest_info(bposd_window *win, int64_t out[3]);

/* Copy one item (BPOSD_WINDOW_OBS ...) of the last bposd_window_run to host memory; bytes must be that item's size. */
int bposd_window_fetch(bposd_window *win, int32_t what, void *host_dst, size_t bytes);

/* Device memory the engine holds: the sum documented at bposd_window_create (the decoders' workspaces are their own). */
int64_t bposd_window_device_bytes(bposd_window *win);

/* Message for the last error on this engine (win == NULL: the last bposd_window_create / bposd_debug_window_step failure). */
const char *bposd_window_last_error(bposd_window *win);

void bposd_window_destroy(bposd_window *win);

/* =====================================================================================================================
 * Circuit-level noise: the columns of a detector error model from a Clifford circuit (csrc/launch_frame.hip, DESIGN.md
 * 4.17; bp_osd_amd/circuit.py holds the circuit description, the host restatement and the reduction to a model).  (No
 * counterpart in the reference.)
 *
 * A circuit is T ops on Q qubits, int32 ops[T][3] = (opcode, a, b); b is read by the two-qubit ops only.  Measurements are
 * numbered in order of appearance.  A fault is a Pauli on one or two qubits in front of op `pos` (pos = T: behind the last
 * op); a Pauli is two bits, bit 0 its X part and bit 1 its Z part (X = 1, Z = 2, Y = 3).  Each fault is propagated on its
 * own as a Pauli frame, one (x, z) bit pair per qubit, all zero at the start:
 *     H    swap x, z                          S    z ^= x
 *     CX   x[b] ^= x[a];  z[a] ^= z[b]        CZ   z[a] ^= x[b];  z[b] ^= x[a]
 *     R, RX   clear both bits                 M / MX   record the flip x[a] / z[a], frame unchanged
 *     MR, MRX record the flip as M / MX, then clear
 * A detector (an observable) is a set of measurements, and its value for a frame the XOR of their flips.  Column i of H
 * (M x F) stacked on L (k x F) is that pair of rows for the frame holding fault i alone.
 *
 * frame_propagate_kernel (csrc/frame_kernels.hip.h) packs 64 faults to a uint64 word, one thread per word; the frames and
 * rows of a chunk of faults live in HBM, word index innermost.  frame_count_kernel and frame_fill_kernel turn the rows into
 * columns (count, prefix sum, fill: deterministic).  Everything is integer and exact.
 */
typedef struct bposd_frame bposd_frame;

enum {
    BPOSD_FRAME_OP_R = 0,   /* reset to |0>            */
    BPOSD_FRAME_OP_RX = 1,  /* reset to |+>            */
    BPOSD_FRAME_OP_M = 2,   /* measure Z               */
    BPOSD_FRAME_OP_MX = 3,  /* measure X               */
    BPOSD_FRAME_OP_MR = 4,  /* measure Z, reset to |0> */
    BPOSD_FRAME_OP_MRX = 5, /* measure X, reset to |+> */
    BPOSD_FRAME_OP_H = 6,
    BPOSD_FRAME_OP_S = 7,
    BPOSD_FRAME_OP_CX = 8, /* a control, b target */
    BPOSD_FRAME_OP_CZ = 9
};

enum { BPOSD_FRAME_DEFAULT = 0, BPOSD_FRAME_OP_BY_OP = 1, BPOSD_FRAME_GROUPS = 2 };

typedef struct {
    int32_t device;          /* HIP device ordinal                                                                  */
    int32_t layered;         /* BPOSD_FRAME_GROUPS (the default): up to 4 ops on disjoint qubits per memory round   */
                             /* trip (frame_propagate_layered_kernel); BPOSD_FRAME_OP_BY_OP: one op at a time       */
    int64_t max_words;       /* most words (of 64 faults) in a chunk; 0: whatever workspace_bytes admits            */
    int64_t workspace_bytes; /* byte budget of a chunk's frames, rows, counts and offsets; 0: 1 GiB                 */
} bposd_frame_config;

/*
 * The annotations arrive inverted: CSR over the n_meas measurements, row i of md_* the detectors (ascending, < M) and of
 * mo_* the observables (ascending, < k) that hold measurement i.  M = 0 or k = 0 is legal.  BPOSD_ERR_INVALID, with the op
 * named (bposd_frame_last_error(NULL)), for an unknown opcode, a qubit outside [0, Q), a == b on a two-qubit op, an n_meas
 * that is not the number of measurements of the op table (an annotation names a measurement out of range), or a table that
 * is not such a CSR.  Everything is copied.
 *
 * Device memory (bposd_frame_device_bytes; every block at least 256 bytes): the tables 4 (3 T + T + 1 + 2 (n_meas + 1) +
 * entries of both CSRs), and from the first bposd_frame_columns on, with wc = min(ceil(F/64), words of a chunk):
 *     13 F                      the faults (pos, qa, qb, Pauli byte);  4 T  the groups of BPOSD_FRAME_GROUPS
 *     8 wc (2 Q + M + k)        frames x, z and rows D, O of a chunk
 *     2 * 2 * 4 * 64 wc         counts and offsets per fault of a chunk, for H and for L
 *     4 * entries               the indices of the chunk with the most column entries
 * The per-call blocks grow and never shrink.
 */
int bposd_frame_create(const bposd_frame_config *cfg, const int32_t *ops, int32_t T, int32_t Q, int32_t n_meas,
                       const int32_t *md_indptr, const int32_t *md_indices, const int32_t *mo_indptr,
                       const int32_t *mo_indices, int32_t M, int32_t k, bposd_frame **out);

/*
 * Propagate F faults (host pointers): pos[F] in 0 .. T and ascending, qa[F], qb[F] (-1: a one-qubit fault; qb == NULL:
 * all of them are), pauli[F] = pa | pb << 2.  The fault index is the position in these arrays.  BPOSD_ERR_INVALID, with the
 * fault named, for pos outside 0 .. T, faults not sorted by pos, a qubit out of range, qa == qb, Pauli code 0 on qa, and
 * Pauli code 0 on a qb that is not -1 (or a code on qb = -1); nothing is launched then.  The faults are cut into chunks of
 * whole words; the last word is ragged, and its padding bits belong to no fault and give no entry.  Synchronous.
 * counts_out (may be NULL) receives the entries of H and of L over the F columns, which is what bposd_frame_fetch needs room
 * for.  Every call starts from zero frames.
 */
int bposd_frame_columns(bposd_frame *fr, const int32_t *pos, const int32_t *qa, const int32_t *qb, const uint8_t *pauli,
                        int64_t F, int64_t counts_out[2]);

/* The columns of the last bposd_frame_columns as CSC over the faults: h_indptr / l_indptr [F + 1], h_indices / l_indices
 * the detectors / observables of every column in ascending order. */
int bposd_frame_fetch(bposd_frame *fr, int64_t *h_indptr, int32_t *h_indices, int64_t *l_indptr, int32_t *l_indices);

/* Device memory the handle holds: the sum documented at bposd_frame_create. */
int64_t bposd_frame_device_bytes(bposd_frame *fr);

/* Message for the last error on this handle (fr == NULL: the last bposd_frame_create failure). */
const char *bposd_frame_last_error(bposd_frame *fr);

void bposd_frame_destroy(bposd_frame *fr);

/* Message for the last error on this handle (h == NULL: last create() failure). */
const char *bposd_last_error(bposd_handle *h);

void bposd_destroy(bposd_handle *h);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* BPOSD_MI355X_H */
