/*
 * bposd_mi355x_debug.h -- diagnostics of libbposd_mi355x.so that have no counterpart in the reference's interface:
 * which kernel ran, the bank-conflict model of its LDS layout, and the layout tables themselves (host only) for the
 * CPU tests.  Not needed to use the decoder; include/bposd_mi355x.h is the drop-in boundary.
 */
#ifndef BPOSD_MI355X_DEBUG_H
#define BPOSD_MI355X_DEBUG_H

#include "bposd_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* Diagnostics: simulated LDS cycles of one bit pass (bank-conflict model) for the natural bit order, the
 * order the library chose, and the conflict-free ideal.  Any pointer may be NULL. */
int bposd_layout_info(bposd_handle *h, int64_t *natural_cycles, int64_t *chosen_cycles, int64_t *ideal_cycles);

/* Diagnostics: which BP kernel the last decode call launched, and the bank-conflict model of its bit pass.
 * kernel: BPOSD_BP_KERNEL_*.  lds_model[4] (local-edge and class kernels, else zeros): modelled ds_read_b64 cycles of one
 * bit pass per workgroup, their conflict-free floor, modelled ds_write_b64 cycles, their floor; after a bp_large_kernel launch
 * lds_model[0] is the form that ran (0: per-edge messages both ways (product-sum); 1: min-sum, one 32-byte record per check in the
 * workspace; 2: min-sum, per-check data in LDS).  Any pointer may be NULL. */
#define BPOSD_BP_KERNEL_LDS 0    /* bp_kernel: every message in LDS, per-lane degree predicates */
#define BPOSD_BP_KERNEL_LOCAL 1  /* bp_local_kernel: (3,6)-regular codes, a third of the messages in registers */
#define BPOSD_BP_KERNEL_CLASS 2  /* bp_class_kernel: one check degree, bits sorted into degree classes */
#define BPOSD_BP_KERNEL_LARGE 3  /* bp_large_kernel: messages in HBM */
#define BPOSD_BP_KERNEL_SERIAL 4 /* bp_serial_kernel: schedule = serial */
#define BPOSD_BP_KERNEL_ANYDEG 5 /* bp_anydeg_kernel: check degree > 16 or bit degree > 8 (run-time degree loops) */
#define BPOSD_BP_KERNEL_RELAY 6  /* bp_relay_kernel: relay mode (bposd_set_relay), any degree */
int bposd_bp_kernel_info(bposd_handle *h, int32_t *kernel, int64_t *lds_model);

/* Diagnostics: the exact kernel instances the last launches of this handle ran (a later change of the dispatch rules shows
 * up here).  bp[6] / osd[6], either may be NULL: [0] the family code -- BPOSD_BP_KERNEL_* for bp, the bposd_last_osd_kernel
 * code for osd (1 osd_kernel, 2 osd_wave_kernel, 3 osd_large_kernel, 4 osd_mw_kernel) -- or -1 before the first launch;
 * [1..4] the instance's template integers in declaration order, zeros where there are fewer; [5] 1 if the kernel read
 * packed syndromes and wrote packed rows.  Template integers per family:
 *   bp_kernel <DC, DV, CPT, MAXNT>          (CPT 1 / MAXNT 1024: shape 1; 2 / 512: shape 2; 4 / 256: shape 4; 2 / 1024: shape 8)
 *   bp_local_kernel <CPT, MP, MINW, EARLY>
 *   bp_class_kernel <DCLO, DC, DVHI, MP>    (DVLO follows from the degree class)
 *   bp_large_kernel <DC, DV, METHOD>
 *   bp_serial_kernel, bp_anydeg_kernel      (no template integers)
 *   bp_relay_kernel <INSTANCE>, threads     (INSTANCE 1: messages, prefixes and M in LDS; 2: in the lane's workspace)
 *   osd_kernel <W>,  osd_wave_kernel <RPL, W>,  osd_mw_kernel <NWV, RPL, W, MINW>,  osd_large_kernel <RPT>
 * The OSD record is also written by the rank probe of an HBM-resident handle at creation. */
int bposd_debug_last_instance(bposd_handle *h, int32_t bp[6], int32_t osd[6]);

/* Diagnostics, host only (needs no device): the ownership / position layout the local-edge BP kernel would use for a
 * (3,6)-regular pcm with n = 2m.  out[16]: modelled ds_read_b64 cycles of one bit pass, their conflict-free
 * floor, positions in select-free (uniform) groups, mixed (group, slot) pairs, positions, nine class sizes, modelled
 * ds_write_b64 cycles of one bit pass, their floor. */
int bposd_debug_local_layout(const int32_t *csr_indptr, const int32_t *csr_indices, int32_t m, int32_t n, int64_t *out);

/* Diagnostics, host only (no handle, no device): how a synchronous host-pointer call of B syndromes is cut into chunks for a
 * handle of `nlanes` lanes on a device of `num_cu` CUs.  n is the block length, read only where per_shot_rows != 0
 * (bposd_decode_batch_rows: ~64 MB of channel rows bound a chunk); large != 0 is an HBM-resident code (at least four
 * workgroups per CU in a chunk); taper != 0 is bposd_decode_batch and its kin (a four-chunk call on four lanes is cut
 * 7 : 7 : 6 : 4), 0 the observables calls (equal chunks).  BPOSD_HOST_CHUNK, read on every call, replaces the target chunk
 * size.  Returns the chunk count (at most 16) and writes count + 1 ascending bounds, bounds[0] = 0 and bounds[count] = B;
 * BPOSD_ERR_INVALID for B outside 1 .. 2^31 - 1, a non-positive n, nlanes or num_cu, or a NULL bounds. */
int bposd_debug_host_chunks(int64_t B, int32_t n, int32_t per_shot_rows, int32_t nlanes, int32_t num_cu, int32_t large, int32_t taper,
                            int64_t *bounds);

/* Diagnostics, host only: the wave pairing of that layout.  The two-checks-per-thread kernels run groups w and w + MP / 128
 * in wave w; groups of equal key (4 * dl(slot 0) + dl(slot 1), 15 = a slot whose lanes differ) are moved into the same wave,
 * which then runs a loop body compiled for that key.  group_key [MP / 64], pos_chk [MP] (check at a position, -1 padding),
 * info[8]: modelled read cycles, write cycles, mixed (group, slot) pairs before the pairing; the same three after it (equal);
 * positions MP; waves whose two groups differ in key (they run the generic body). */
int bposd_debug_local_keys(const int32_t *csr_indptr, const int32_t *csr_indices, int32_t m, int32_t n, int32_t *group_key,
                           int32_t *pos_chk, int64_t *info);

/* Diagnostics, host only: which loop body every wave of that pairing runs.  A wave whose groups share a key runs that key's
 * body; a wave (uniform key k, mixed group) runs the pair body 32 + k of the kernel instance compiled with PAIRKEY = k, which
 * the host then launches (one k per instance: the layout's most frequent); every other wave of unequal groups runs the generic
 * body.  wave_body [MP / 128]: a group key, a pair key, or -1 (generic).  info[4]: positions MP; PAIRKEY of the instance
 * (-1: the plain one); waves on the generic body; mode (2 pair body; 0 generic / 1 uniform group demoted to mixed are
 * measurement settings of BPOSD_PAIR_MODE). */
int bposd_debug_local_waves(const int32_t *csr_indptr, const int32_t *csr_indices, int32_t m, int32_t n, int32_t *wave_body,
                            int64_t *info);

/* Diagnostics: PAIRKEY of the bp_local_kernel instance the last BP launch of this handle ran; -1 for the plain instance and
 * after a launch of another kernel family. */
int bposd_debug_last_pair_key(bposd_handle *h, int32_t *pair_key);

/* Diagnostics: park at drain of the local-edge BP kernel (csrc/local_park.h).  mode 0 = auto (a device-pointer call with an
 * OSD stage parks its unfinished shots once its queue is dry, if another lane of the handle has work in flight), 1 = never,
 * 2 = force: every call the kernel can park in does, and every shot that reaches its first chunk boundary parks there
 * whatever the queue says -- a test then depends on no timing.  BPOSD_PARK=0|1|force in the environment wins (0 = never). */
int bposd_debug_set_park(bposd_handle *h, int32_t mode);

/* Diagnostics: the number of park records the last call queued on `lane` wrote (0 where it did not park).  Waits for that
 * lane; valid until the lane's next call. */
int bposd_debug_last_parked(bposd_handle *h, int32_t lane, int32_t *parked);

/* Diagnostics: how often the handle has launched lsd_kernel<false> (launches[0], LSD-0) and lsd_kernel<true> (launches[1],
 * a sweep or growth for free bits). */
int bposd_debug_lsd_launches(bposd_handle *h, int64_t launches[2]);

/* Diagnostics: duration of obs_kernel in the last observables call queued on `lane` (HIP events on the lane's stream; waits
 * for that lane), or, lane = -1, summed over the chunks of the last synchronous host-pointer observables call.  obs_kernel
 * runs behind the events of bposd_last_timing / bposd_lane_timing: their bp_ms and osd_ms do not include it. */
int bposd_debug_obs_timing(bposd_handle *h, int32_t lane, double *obs_ms);

/* Diagnostics: durations of dem_sample_kernel and dem_score_kernel in the engine's last batch (HIP events on the engine's
 * stream; the batch has been waited for).  score_ms is 0 after bposd_dem_sample.  Either pointer may be NULL. */
int bposd_debug_dem_timing(bposd_dem *dem, double *sample_ms, double *score_ms);

/* Diagnostics: the harvest kernels alone (bposd_dem_set_harvest must be on), with no sampler, decoder or scorer involved.
 * Every pointer is a HOST pointer: fault_words [B][ceil(N/64)] (padding bits zero) go into the engine's fault rows;
 * corrections are [B][ceil(N/64)] words (packed != 0, padding bits zero) or [B][N] bytes of which bit 0 counts -- the two
 * forms a decoder leaves its rows in; select[b] != 0 stands in for the flag test.  1 <= B <= capacity.  Waits, and leaves
 * bposd_dem_harvest_info and items 0 and 11 .. 15 of bposd_dem_fetch as a batch of B shots would. */
int bposd_debug_dem_harvest(bposd_dem *dem, const uint64_t *fault_words, const void *corrections, int32_t packed,
                            const uint8_t *select, int64_t B);

/* Diagnostics: duration of the three harvest launches of the engine's last batch (HIP events on the engine's stream; the
 * batch has been waited for).  Refused unless that batch ran with the harvest on. */
int bposd_debug_dem_harvest_timing(bposd_dem *dem, double *harvest_ms);

/* Diagnostics: fault_sums_kernel alone (bposd_dem_fault_sums of the public header), with no sampler, decoder or scorer
 * involved.  Every pointer is a HOST pointer: fault_words [B][ceil(N/64)] (padding bits zero) go into the engine's fault
 * rows.  select_bytes [B] (row b is selected when select_bytes[b] != 0) go through harvest_list_kernel first, so that the
 * kernel reads the list and the count it reads in production (bposd_dem_set_harvest must be on); mult is then [F], one per
 * selected row in ascending row order.  select_bytes == NULL selects every row the implicit way (BPOSD_DEM_SELECT_ALL);
 * mult is then [B].  mult and sums go together, as there; counts [N] and sums [N].  1 <= B <= capacity.  Waits, and leaves
 * item 0 of bposd_dem_fetch as a batch of B shots would (nothing else: the harvest's items are gone). */
int bposd_debug_dem_fault_sums(bposd_dem *dem, const uint64_t *fault_words, const uint8_t *select_bytes,
                               const uint32_t *mult, int64_t B, uint64_t *counts, uint64_t *sums);

/* Diagnostics: duration of the last fault_sums_kernel launch (HIP events on the engine's stream; the call has waited).
 * Refused when the last call selected no row, or there was none. */
int bposd_debug_dem_fault_sums_timing(bposd_dem *dem, double *sums_ms);

/* Diagnostics: one window_step_kernel launch on rows the caller supplies, with no decoder and no engine involved -- the
 * commit of one window from `decoded` and the gather of the next into `syndrome`.  Every pointer is a HOST pointer; rows
 * go up, the kernel runs on `device`, rows come back.  H, L as bposd_dem_tables takes them.  Commit entry c is position
 * commit_pos[c] (ascending, < decoded_cols) of a decoded row and global fault commit_fault[c] (ascending); decoded holds B
 * rows of decoded_cols bytes, or (decoded_packed) of ceil(decoded_cols/64) words.  gather_det[n_gather] ascends; syndrome
 * receives B rows of n_gather bytes or (syndrome_packed) of ceil(n_gather/64) words.  running [B][ceil(M/64)], observables
 * [B][ceil(k/64)], correction [B][ceil(N/64)] (may be NULL), conv_all uint8[B] and iters int32[B] are read and written
 * in place; prev_converged / prev_iters [B] may be NULL.  n_commit = 0 is a gather-only step (decoded may be NULL),
 * n_gather = 0 a commit-only one (syndrome may be NULL).  word_range receives the staged detector words [w_lo, w_hi). */
typedef struct {
    int32_t device, M, N, k;
    const int32_t *h_indptr, *h_indices, *l_indptr, *l_indices;
    int64_t B;
    int32_t n_commit;
    const int32_t *commit_pos, *commit_fault;
    int32_t decoded_cols, decoded_packed;
    const void *decoded;
    const uint8_t *prev_converged;
    const int32_t *prev_iters;
    int32_t n_gather;
    const int32_t *gather_det;
    int32_t syndrome_packed;
    void *syndrome;
    uint64_t *running, *observables, *correction;
    uint8_t *conv_all;
    int32_t *iters;
    int32_t word_range[2];
} bposd_window_step_args;
int bposd_debug_window_step(bposd_window_step_args *args);

/* Diagnostics: the durations of the window_step_kernel launches of the engine's last batch, summed, and of
 * window_score_kernel (HIP events on the engine's stream; waits for the batch).  score_ms is 0 after a decode call.  Either
 * pointer may be NULL. */
int bposd_debug_window_timing(bposd_window *win, double *step_ms, double *score_ms);

/* Diagnostics: the durations of the last bposd_frame_columns call's frame_propagate_kernel, frame_count_kernel and
 * frame_fill_kernel launches, each summed over the chunks (HIP events on the handle's stream; the call has waited), in
 * ms[3]; info[2] = the chunks of that call, and the kernel launches of the handle so far (a refused call adds none).
 * Either pointer may be NULL; ms is refused before the first successful call. */
int bposd_debug_frame_timing(bposd_frame *fr, double ms[3], int64_t info[2]);

/* Diagnostics, host only: the tables bp_class_kernel would run with for a pcm whose check and bit degrees fall inside one
 * compiled instance -- (check degrees; bit degrees) = (7; 3..4), (6; 3), (4; 2), (8; 4), (3..4; 1..2) -- and
 * BPOSD_ERR_UNSUPPORTED otherwise.  info[11]: highest check degree, lowest / highest bit degree, bit slots per thread, LDS
 * stride MP, threads per workgroup, modelled read cycles of one bit pass and their floor, modelled write cycles and their
 * floor, lowest check degree.  Nullable outputs: pos_chk [MP], pos_bit [slots * MP], bit_slot [DVHI * slots * MP],
 * grp_deg [slots * MP / 64], grp_cdeg [MP / 64] -- callers size them for MP = 1024, 2 slots, DVHI = 4. */
int bposd_debug_class_layout(const int32_t *csr_indptr, const int32_t *csr_indices, int32_t m, int32_t n, int32_t *pos_chk,
                             int32_t *pos_bit, int32_t *bit_slot, int32_t *grp_deg, int32_t *grp_cdeg, int64_t *info);

/* Diagnostics: csrc/portable_math.h evaluated ON THE DEVICE, one thread per element -- the routines the product-sum kernels
 * inline, so that a test can compare the gfx950 compile of that header with a host compile bit for bit.  a, b, y are host
 * pointers to `count` doubles (count <= 2^28; b is read by which = 4 only and may be NULL otherwise).  y[i] =
 *   0 pm_tanh(a)   1 pm_log(a)   2 pm_expm1(a)   3 pm_tanh_half(a)   4 pm_log_quot(a, b)
 *   5 / 6 pm_ps_tanh_half(a, 0 / 1)   7 / 8 pm_ps_log_ratio(a, 0 / 1)
 * Runs on the current device; needs no handle. */
int bposd_debug_portable_math(int32_t which, const double *a, const double *b, double *y, int64_t count);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BPOSD_MI355X_DEBUG_H */
