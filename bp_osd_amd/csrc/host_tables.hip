// host_tables.hip -- host side of libbposd_mi355x.so, what bposd_create runs once per code: GF(2) rank, priors, the
// Tanner-graph tables of every BP kernel family with their layout searches (local_layout.h, class_layout.h), the rank
// probe of large codes, and the host-only bposd_debug_* exports that report those layouts without a device.
// The decode calls are in bposd_capi.hip (device pointers) and decode_host.hip (host pointers); the declarations shared with
// them are in internal.h.
#include "internal.h"

#include <climits>
#include <cmath>

#include "local_layout.h"
#include "class_layout.h"

using namespace bposd;
using namespace bposd_host;

namespace bposd_host {
// GF(2) rank of the pcm by packed elimination (ctor-time, host).  a1: upstream's ctor
// eliminates H once to learn rank and k' = n - rank.
int gf2_rank_host(int m, int n, const std::vector<int>& rp, const std::vector<int>& ci) {
    const int W = (n + 63) / 64;
    std::vector<uint64_t> a((size_t)m * W, 0);
    for (int r = 0; r < m; ++r)
        for (int e = rp[r]; e < rp[r + 1]; ++e) a[(size_t)r * W + (ci[e] >> 6)] |= 1ull << (ci[e] & 63);
    int rank = 0;
    for (int j = 0; j < n && rank < m; ++j) {
        const int w = j >> 6;
        const uint64_t bit = 1ull << (j & 63);
        int p = -1;
        for (int r = rank; r < m; ++r)
            if (a[(size_t)r * W + w] & bit) { p = r; break; }
        if (p < 0) continue;
        if (p != rank)
            for (int x = 0; x < W; ++x) std::swap(a[(size_t)p * W + x], a[(size_t)rank * W + x]);
        for (int r = rank + 1; r < m; ++r)
            if (a[(size_t)r * W + w] & bit)
                for (int x = w; x < W; ++x) a[(size_t)r * W + x] ^= a[(size_t)rank * W + x];
        ++rank;
    }
    return rank;
}

// One int table on the device.  A table that exists is freed first: the LDS kernel's tables are rebuilt when the workgroup
// shape changes, and bposd_set_bp_variant(64) builds the serial tables on a handle that may have none yet.
int upload_ints(bposd_handle* h, DevArray<int>& dst, const std::vector<int>& v) {
    HIP_TRY(h, dst.alloc(sizeof(int) * std::max<size_t>(v.size(), 1)));
    HIP_TRY(h, hipMemcpy(dst, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice));
    return 0;
}

const DegPair kPairs[] = {{4, 2}, {6, 3}, {8, 4}, {12, 6}, {16, 8}};

bool pick_pair(int dc, int dv, DegPair* out) {
    for (const auto& p : kPairs)
        if (p.dc >= dc && p.dv >= dv) { *out = p; return true; }
    return false;
}

// The one place that turns error probabilities into what the kernels read (bposd_channel_tables):
// a3: prior LLR = log((1 - p) / p), a11: weight = log(1 / p), evaluated on the host in fp64 (same libm call the CPU path
// makes) so that device arithmetic is add / compare / multiply only.  The handle's channel, the alternative channel and
// the per-shot rows all come from here, which is what makes a row equal update_channel_probs with that row bit for bit.
// Either output may be null.  Returns the index of the first value that is no probability + 1, 0 if there is none.
int64_t first_bad_prob(const double* probs, int64_t count) {
    for (int64_t i = 0; i < count; ++i)
        if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return i + 1;
    return 0;
}

int64_t channel_tables(const double* probs, int64_t count, double* prior_llr, double* cost) {
    if (const int64_t bad = first_bad_prob(probs, count)) return bad;
    if (prior_llr)
        for (int64_t i = 0; i < count; ++i) prior_llr[i] = std::log((1 - probs[i]) / probs[i]);
    if (cost)
        for (int64_t i = 0; i < count; ++i) cost[i] = std::log(1 / probs[i]);
    return 0;
}

int upload_priors(bposd_handle* h) {
    std::vector<double> l0(h->n), cost(h->n);
    if (channel_tables(h->probs.data(), h->n, l0.data(), cost.data())) return fail(h, BPOSD_ERR_INVALID, "channel_probs holds a value that is not a probability");
    HIP_TRY(h, hipMemcpy(h->d_llr0, l0.data(), sizeof(double) * h->n, hipMemcpyHostToDevice));
    h->probs_uniform = true;
    for (int i = 1; i < h->n; ++i)
        if (h->probs[i] != h->probs[0]) { h->probs_uniform = false; break; }
    // a11: weight(x) = sum over set bits of log(1/p_i) (ldpc v2).  For a uniform 0 < p < 1 every term is
    // the same positive number, so the sums order candidates exactly like Hamming weights (identical
    // partial sums, strictly increasing in the count) and the integer path is used.
    HIP_TRY(h, hipMemcpy(h->d_cost, cost.data(), sizeof(double) * h->n, hipMemcpyHostToDevice));
    h->fp_weights = (h->cfg.weight_fn == 0) &&
                    !(h->probs_uniform && h->probs[0] > 0.0 && h->probs[0] < 1.0);
    return 0;
}
// ---------------------------------------------------------------------------------------------
// Bit-pass layout.  The check pass is bank-conflict free by construction (lane c <-> slot k*MP + c).
// The bit pass gathers/scatters slot (k*MP + c) for the d-th edge of each of 64 lanes; its conflicts
// depend only on which bits share a 32-lane (ds_read_b64: 64 banks) / 16-lane (ds_write_b64: 32 banks)
// group.  The order of bits over lanes is free (tables are position-indexed), so the host simulates
// the LDS cycles (MI355X_MICROARCH.md §LDS banking model) of a family of orders -- natural, and
// two-block orders where each block of (outer x inner) bits is laid out inner-major or outer-major with
// groups padded to a multiple of 32 lanes (the shapes hypergraph-product codes have) -- and keeps the
// cheapest.  For H1922 (31x31 | 31x31) the outer-major order of the first block is conflict free.
struct EdgeSlot { int slot; };

static long bit_pass_cycles(const std::vector<int>& bit_of_pos, int NP, int NT, int VPT, int dv_max,
                            const std::vector<int>& cptr, const std::vector<int>& eslot, long stop_at) {
    long total = 0;
    int cnt[64];
    int first[64];
    for (int r = 0; r < VPT; ++r) {
        for (int w0 = 0; w0 < NT; w0 += 64) {
            for (int d = 0; d < dv_max; ++d) {
                int slots[64];
                bool any = false;
                for (int l = 0; l < 64; ++l) {
                    const int p = r * NT + w0 + l;
                    const int i = p < NP ? bit_of_pos[p] : -1;
                    slots[l] = (i >= 0 && cptr[i] + d < cptr[i + 1]) ? eslot[cptr[i] + d] : -1;
                    any |= slots[l] >= 0;
                }
                if (!any) continue;
                // reads: two 32-lane groups, an 8-byte access covers banks 2*slot, 2*slot+1 of 64
                for (int g = 0; g < 64; g += 32) {
                    int worst = 0;
                    for (int b = 0; b < 32; ++b) { cnt[b] = 0; first[b] = -1; }
                    for (int l = g; l < g + 32; ++l) {
                        if (slots[l] < 0) continue;
                        const int b = slots[l] & 31;
                        // distinct addresses on the same bank serialise (identical ones broadcast; cannot
                        // happen here: every edge has its own slot)
                        ++cnt[b];
                        worst = std::max(worst, cnt[b]);
                    }
                    total += std::max(worst, 1);
                }
                // writes: four 16-lane groups, 32 banks -> 16 slot classes
                for (int g = 0; g < 64; g += 16) {
                    int worst = 0;
                    for (int b = 0; b < 16; ++b) cnt[b] = 0;
                    for (int l = g; l < g + 16; ++l) {
                        if (slots[l] < 0) continue;
                        const int b = slots[l] & 15;
                        ++cnt[b];
                        worst = std::max(worst, cnt[b]);
                    }
                    total += std::max(worst, 1);
                }
                if (total >= stop_at) return total;
            }
        }
    }
    return total;
}

static int round32(int x) { return (x + 31) / 32 * 32; }

// positions of a block of `count` bits starting at bit `b0`, viewed as outer x inner with the given inner
// size, laid out inner-major (transposed = false) or outer-major (transposed = true), groups padded to 32
static int place_block(std::vector<int>& bit_of_pos, int p0, int b0, int count, int inner, bool transposed, int NP) {
    if (count == 0) return p0;
    if (inner <= 0 || count % inner != 0) return -1;
    const int outer = count / inner;
    const int gsz = transposed ? round32(outer) : round32(inner);
    const int ngr = transposed ? inner : outer;
    if ((long)p0 + (long)gsz * ngr > NP) return -1;
    for (int a = 0; a < outer; ++a)
        for (int b = 0; b < inner; ++b) {
            const int p = transposed ? p0 + b * gsz + a : p0 + a * gsz + b;
            bit_of_pos[p] = b0 + a * inner + b;
        }
    return p0 + gsz * ngr;
}

static void choose_bit_layout(bposd_handle* h, int MP, int NT, int VPT, std::vector<int>& best_bit_of_pos) {
    const int n = h->n, NP = NT * VPT;
    // CSC view with the LDS slot of every edge
    std::vector<int> cptr(n + 1, 0), fill(n, 0);
    for (int e = 0; e < h->E; ++e) cptr[h->ci[e] + 1]++;
    for (int i = 0; i < n; ++i) cptr[i + 1] += cptr[i];
    std::vector<int> eslot(h->E);
    for (int c = 0; c < h->m; ++c)
        for (int e = h->rp[c]; e < h->rp[c + 1]; ++e) {
            const int i = h->ci[e];
            eslot[cptr[i] + fill[i]++] = (e - h->rp[c]) * MP + c;  // ascending row within a column
        }
    std::vector<int> cand(NP, -1);
    for (int i = 0; i < n; ++i) cand[i] = i;
    long best = bit_pass_cycles(cand, NP, NT, VPT, h->dv_max, cptr, eslot, LONG_MAX);
    best_bit_of_pos = cand;
    h->layout_cost_natural = best;
    // ideal: every instruction that touches a real bit costs 2 read + 4 write group-cycles
    long ninstr = 0;
    for (int r = 0; r < VPT; ++r)
        for (int w0 = 0; w0 < NT; w0 += 64)
            if (r * NT + w0 < n) ninstr += h->dv_max;
    h->layout_cost_ideal = ninstr * 6;
    if (best <= h->layout_cost_ideal + h->layout_cost_ideal / 20) { h->layout_cost = best; return; }
    // two-block family: bits [0, s) as (s/p1 x p1), bits [s, n) as ((n-s)/p2 x p2)
    for (int p1 = 2; p1 <= 64; ++p1) {
        for (int o1 = 0; o1 <= 64 && o1 * p1 <= n; ++o1) {
            const int s0 = o1 * p1;
            const int rest = n - s0;
            for (int p2 = 2; p2 <= 64; ++p2) {
                if (rest % p2 != 0 || rest / p2 > 64) continue;
                if (s0 == 0 && p1 != 2) continue;  // a single block: p1 is irrelevant, visit once
                for (int t = 0; t < 4; ++t) {
                    std::fill(cand.begin(), cand.end(), -1);
                    int q = place_block(cand, 0, 0, s0, p1, (t & 1) != 0, NP);
                    if (q < 0) continue;
                    q = place_block(cand, q, s0, rest, p2, (t & 2) != 0, NP);
                    if (q < 0) continue;
                    const long c = bit_pass_cycles(cand, NP, NT, VPT, h->dv_max, cptr, eslot, best);
                    if (c < best) { best = c; best_bit_of_pos = cand; }
                }
            }
        }
    }
    h->layout_cost = best;
}

int build_tables(bposd_handle* h, int DC, int DV, int MP, int NT, int VPT) {
    // LDS slot of the k-th edge of check c is k * MP + c (MP = checks padded to threads x CPT)
    const int m = h->m, n = h->n, NP = NT * VPT;
    std::vector<int> bit_of_pos;
    choose_bit_layout(h, MP, NT, VPT, bit_of_pos);
    std::vector<int> pos_of_bit(n, -1);
    for (int p = 0; p < NP; ++p)
        if (bit_of_pos[p] >= 0) pos_of_bit[bit_of_pos[p]] = p;
    std::vector<int> chk_deg(m), var_deg(NP, 0);
    std::vector<int> var_pos((size_t)DV * NP, 0);
    for (int c = 0; c < m; ++c) {
        chk_deg[c] = h->rp[c + 1] - h->rp[c];
        for (int e = h->rp[c]; e < h->rp[c + 1]; ++e) {
            const int k = e - h->rp[c];
            const int p = pos_of_bit[h->ci[e]];
            const int d = var_deg[p]++;  // rows visited ascending => ascending row within a column
            var_pos[(size_t)d * NP + p] = k * MP + c;
        }
    }
    int rc;
    if ((rc = upload_ints(h, h->d_chk_deg, chk_deg))) return rc;
    if ((rc = upload_ints(h, h->d_var_deg, var_deg))) return rc;
    if ((rc = upload_ints(h, h->d_var_pos, var_pos))) return rc;
    if ((rc = upload_ints(h, h->d_pos_bit, bit_of_pos))) return rc;
    h->tab_dc = DC;
    h->tab_dv = DV;
    h->tab_mp = MP;
    h->tab_np = NP;
    return 0;
}
// Admission test of the local-edge BP kernel, for bposd_create and the host-only diagnostics alike: a (3,6)-regular pcm
// with n = 2m and at most 2048 checks for which the search finds a layout.  BPOSD_OK and the graph, the layout and the
// number of positions MP, or the reason there is none.
struct LocalLayout {
    int MP = 0;
    local_layout::Graph g;
    local_layout::Layout best;
};
int local_layout_for(const int32_t* indptr, const int32_t* indices, int m, int n, bool pair, LocalLayout& out) {
    if (n != 2 * m) return BPOSD_ERR_INVALID;
    std::vector<int> rp(indptr, indptr + m + 1), ci(indices, indices + indptr[m]);
    out.MP = m <= 1024 ? 1024 : 2048;  // the kernels are compiled for 1024 (H1922: 961 checks) and 2048 positions
    if (m > out.MP) return BPOSD_ERR_UNSUPPORTED;
    for (int c = 0; c < m; ++c)
        if (rp[c + 1] - rp[c] != 6) return BPOSD_ERR_UNSUPPORTED;
    std::vector<int> deg(n, 0);
    for (int e : ci) {
        if (e < 0 || e >= n) return BPOSD_ERR_INVALID;
        deg[e]++;
    }
    for (int i = 0; i < n; ++i)
        if (deg[i] != 3) return BPOSD_ERR_UNSUPPORTED;
    return local_layout_host(rp, ci, m, n, out.MP, out.g, out.best, pair) ? BPOSD_OK : BPOSD_ERR_UNSUPPORTED;
}

int build_tables_local(bposd_handle* h) {
    using namespace local_layout;
    h->local_ok = false;
    const int m = h->m;
    LocalLayout ll;
    if (local_layout_for(h->rp.data(), h->ci.data(), m, h->n, true, ll)) return 0;
    const int MP = ll.MP;
    const Graph& g = ll.g;
    const Layout& best = ll.best;
    if (getenv("BPOSD_DEBUG_OCC"))
        fprintf(stderr, "[bposd] local-edge layout: bit pass %lld read cycles (floor %d) + %lld write cycles (floor %d), %d mixed pairs, %d uniform positions\n",
                best.passes, 4 * (MP / 32), best.wcycles, 6 * 4 * (MP / 64), best.mixed, best.nfull);
    h->local_passes = best.passes;
    h->local_wcycles = best.wcycles;

    // ---- tables
    const std::vector<int>&owner = best.owner, &load = best.load, &pos_of = best.pos_of, &pos_chk = best.pos_chk;
    const WavePlan plan = wave_plan(g, best, pair_mode());  // which body every wave runs; the instance that has them
    const std::vector<int>& grp_dl = plan.grp_dl;
    h->local_pair_key = plan.pair_key;
    if (getenv("BPOSD_DEBUG_OCC")) {
        fprintf(stderr, "[bposd] wave bodies (-1 generic):");
        for (int b : plan.body) fprintf(stderr, " %d", b);
        fprintf(stderr, "; instance PAIRKEY %d, %d generic wave(s)\n", plan.pair_key, plan.generic);
    }
    // LDS slot of (check c, bit i) for the check's four non-local edges, ascending column order
    auto slot_of = [&](int c, int i) {
        int k = 0;
        for (int e = h->rp[c]; e < h->rp[c + 1]; ++e) {
            const int j = h->ci[e];
            if (owner[j] == c) continue;
            if (j == i) return k * MP + pos_of[c];
            ++k;
        }
        return -1;
    };
    // Padding positions (pos_chk < 0): the two "bits" of such a position are wired to the position's own four LDS slots
    // (slot k * MP + p), a closed toy graph that needs no predicate in the kernel (bp_local_kernel.hip.h).
    std::vector<int> pos_bit(2 * (size_t)MP, -1), pos_alo(2 * (size_t)MP, 0), pos_ahi(2 * (size_t)MP, 0), pos_dl(2 * (size_t)MP, 0);
    for (int p = 0; p < MP; ++p)
        for (int b = 0; b < 2; ++b) {
            pos_alo[(size_t)b * MP + p] = (2 * b) * MP + p;
            pos_ahi[(size_t)b * MP + p] = (2 * b + 1) * MP + p;
        }
    for (int c = 0; c < m; ++c) {
        const int p = pos_of[c];
        for (int b = 0; b < 2; ++b) {
            const int i = load[2 * c + b];
            int o[2];
            g.others(i, c, o);
            const int sx = slot_of(o[0], i), sy = slot_of(o[1], i);
            if (sx < 0 || sy < 0) return 0;
            pos_dl[(size_t)b * MP + p] = g.rank_of(i, c);
            pos_bit[(size_t)b * MP + p] = i;
            pos_alo[(size_t)b * MP + p] = sx;
            pos_ahi[(size_t)b * MP + p] = sy;
        }
    }
    int rc;
    if ((rc = upload_ints(h, h->d_lpos_chk, pos_chk))) return rc;
    if ((rc = upload_ints(h, h->d_lpos_bit, pos_bit))) return rc;
    if ((rc = upload_ints(h, h->d_lpos_alo, pos_alo))) return rc;
    if ((rc = upload_ints(h, h->d_lpos_ahi, pos_ahi))) return rc;
    if ((rc = upload_ints(h, h->d_lgrp_dl, grp_dl))) return rc;
    if ((rc = upload_ints(h, h->d_lpos_dl, pos_dl))) return rc;
    h->local_mp = MP;
    h->local_ok = true;
    return 0;
}
// ------------------------------------------------------------------ class BP kernel: tables + launch
// Instances: (check degrees; bit degrees) = (7; 3..4) -- the reference's three example codes --, (6; 3) -- H1922 with
// product-sum, other (3,6)-regular codes --, (4; 2) -- toric codes, hgp(ring_code) --, (8; 4), and (3..4; 1..2) -- surface
// codes, hgp(rep_code) --; LDS stride 256 / 512 / 1024, two bit slots per thread.
struct ClassShape { int dclo, dc, dvlo, dvhi; };
const ClassShape kClassShapes[] = {{7, 7, 3, 4}, {6, 6, 3, 3}, {4, 4, 2, 2}, {8, 8, 4, 4}, {3, 4, 1, 2}};
constexpr int kClassVPT = 2;

// the first instance whose degree ranges cover the code's, or null
const ClassShape* class_shape_for(const std::vector<int>& rp, const std::vector<int>& ci, int m, int n) {
    int clo = 1 << 30, chi = 0, lo = 1 << 30, hi = 0;
    for (int c = 0; c < m; ++c) {
        const int d = rp[c + 1] - rp[c];
        clo = std::min(clo, d); chi = std::max(chi, d);
    }
    std::vector<int> vdeg(n, 0);
    for (int e : ci) vdeg[e]++;
    for (int d : vdeg) { lo = std::min(lo, d); hi = std::max(hi, d); }
    for (const auto& k : kClassShapes)
        if (k.dclo <= clo && chi <= k.dc && k.dvlo <= lo && hi <= k.dvhi) return &k;
    return nullptr;
}

// annealing steps of the class layout search: bposd_create and the host-only bposd_debug_class_layout take the same
// number, so that the diagnostic reports the tables (and the stride) the kernel runs with
static int class_layout_iters() { return getenv("BPOSD_LAYOUT_ITERS") ? atoi(getenv("BPOSD_LAYOUT_ITERS")) : 200000; }

int build_tables_class(bposd_handle* h) {
    h->class_ok = false;
    if (h->bp_hbm || h->m > 1024) return 0;
    const ClassShape* shp = class_shape_for(h->rp, h->ci, h->m, h->n);
    if (!shp) return 0;
    class_layout::Tables T;
    bool ok = false;
    int MP = 0;
    const int iters = class_layout_iters();
    for (int mp : {256, 512, 1024}) {
        if (h->m > mp) continue;
        if (class_layout::build(h->rp, h->ci, h->m, h->n, shp->dclo, shp->dc, shp->dvlo, shp->dvhi, kClassVPT, mp, mp, iters, T)) { ok = true; MP = mp; break; }
    }
    if (!ok) return 0;
    if (getenv("BPOSD_DEBUG_OCC"))
        fprintf(stderr, "[bposd] class BP layout: %d threads, stride %d, bit pass %ld read cycles (floor %ld) + %ld write cycles (floor %ld)\n", T.NT,
                MP, T.read_cycles, T.read_floor, T.write_cycles, T.write_floor);
    int rc;
    if ((rc = upload_ints(h, h->d_cpos_chk, T.pos_chk))) return rc;
    if ((rc = upload_ints(h, h->d_cpos_bit, T.pos_bit))) return rc;
    if ((rc = upload_ints(h, h->d_cbit_slot, T.bit_slot))) return rc;
    if ((rc = upload_ints(h, h->d_cgrp_deg, T.grp_deg))) return rc;
    if ((rc = upload_ints(h, h->d_cgrp_cdeg, T.grp_cdeg))) return rc;
    h->class_dclo = shp->dclo; h->class_dc = shp->dc; h->class_dvlo = shp->dvlo; h->class_dvhi = shp->dvhi; h->class_mp = MP; h->class_nt = T.NT;
    h->class_read_cycles = T.read_cycles; h->class_write_cycles = T.write_cycles;
    h->class_read_floor = T.read_floor; h->class_write_floor = T.write_floor;
    h->class_ok = true;
    return 0;
}
// ------------------------------------------------------------------------ large-code BP launch
int build_tables_large(bposd_handle* h, int DV, int MP) {
    const int m = h->m, n = h->n;
    std::vector<int> chk_deg(m), var_deg(n, 0);
    std::vector<int> var_pos((size_t)DV * n, 0), var_ck((size_t)DV * n, 0);
    for (int c = 0; c < m; ++c) {
        chk_deg[c] = h->rp[c + 1] - h->rp[c];
        for (int e = h->rp[c]; e < h->rp[c + 1]; ++e) {
            const int i = h->ci[e];
            const int d = var_deg[i]++;
            var_pos[(size_t)d * n + i] = (e - h->rp[c]) * MP + c;
            var_ck[(size_t)d * n + i] = c * 16 + (e - h->rp[c]);  // (slot < 16: the large-code kernels are built for check degree <= 16)
        }
    }
    int rc;
    if ((rc = upload_ints(h, h->d_chk_deg, chk_deg))) return rc;
    if ((rc = upload_ints(h, h->d_var_deg, var_deg))) return rc;
    if ((rc = upload_ints(h, h->d_var_pos, var_pos))) return rc;
    if ((rc = upload_ints(h, h->d_var_ck, var_ck))) return rc;
    h->tab_mp = MP;
    return 0;
}
// ------------------------------------------------------------------ serial-schedule BP: tables + launch
int build_tables_serial(bposd_handle* h) {
    const int m = h->m, n = h->n, E = h->E;
    std::vector<int> cp(n + 1, 0), ce(E), erow(E), fill(n, 0);
    for (int e = 0; e < E; ++e) cp[h->ci[e] + 1]++;
    for (int i = 0; i < n; ++i) cp[i + 1] += cp[i];
    for (int c = 0; c < m; ++c)
        for (int e = h->rp[c]; e < h->rp[c + 1]; ++e) {
            erow[e] = c;
            ce[cp[h->ci[e]] + fill[h->ci[e]]++] = e;  // ascending row within a column
        }
    // level(j) = 1 + the highest level among the earlier bits that share a check with j
    std::vector<int> last(m, 0), level(n, 0);
    int nlev = 0;
    for (int i = 0; i < n; ++i) {
        int lv = 0;
        for (int k = cp[i]; k < cp[i + 1]; ++k) lv = std::max(lv, last[erow[ce[k]]]);
        level[i] = lv + 1;
        for (int k = cp[i]; k < cp[i + 1]; ++k) last[erow[ce[k]]] = lv + 1;
        nlev = std::max(nlev, lv + 1);
    }
    std::vector<int> lptr(nlev + 1, 0), lbits(n);
    for (int i = 0; i < n; ++i) lptr[level[i]]++;  // level l (1-based) counted into slot l
    for (int l = 0; l < nlev; ++l) lptr[l + 1] += lptr[l];
    {
        std::vector<int> pos(lptr.begin(), lptr.end() - 1);
        for (int i = 0; i < n; ++i) lbits[pos[level[i] - 1]++] = i;  // ascending bit index inside a level
    }
    int rc;
    if ((rc = upload_ints(h, h->d_cp, cp))) return rc;
    if ((rc = upload_ints(h, h->d_ce, ce))) return rc;
    if ((rc = upload_ints(h, h->d_erow, erow))) return rc;
    if ((rc = upload_ints(h, h->d_lvl_ptr, lptr))) return rc;
    if ((rc = upload_ints(h, h->d_lvl_bits, lbits))) return rc;
    h->nlevels = nlev;
    return 0;
}
// The CSC edge map the CSR-edge kernels walk (any-degree as a forced variant, relay): a handle of the tuned kernels has none
// until one of them is asked for.  Earlier calls may still be running on the handle's lanes.
int ensure_csc_tables(bposd_handle* h) {
    if (h->d_cp) return 0;
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    const int rc = sync_all_lanes(h);
    return rc ? rc : build_tables_serial(h);
}

// LSD mode (lsd_kernel): H by column -- the checks of every bit, ascending -- next to the CSR copy every handle has
int build_tables_lsd(bposd_handle* h) {
    const int m = h->m, n = h->n, E = h->E;
    std::vector<int> cp(n + 1, 0), cr(E), fill(n, 0);
    for (int e = 0; e < E; ++e) cp[h->ci[e] + 1]++;
    for (int i = 0; i < n; ++i) cp[i + 1] += cp[i];
    for (int c = 0; c < m; ++c)
        for (int e = h->rp[c]; e < h->rp[c + 1]; ++e) cr[cp[h->ci[e]] + fill[h->ci[e]]++] = c;
    int rc;
    if ((rc = upload_ints(h, h->d_lsd_cp, cp))) return rc;
    return upload_ints(h, h->d_lsd_cr, cr);
}
// rank of a large code: one elimination of the zero syndrome on the device (the host routine is O(m^2 n / 64))
int probe_rank_large(bposd_handle* h, const DecodeCall& call, int* rank) {
    DevBuf tmp;
    const size_t n = h->n, m = h->m;
    const size_t off_llr = 0, off_synd = off_llr + sizeof(double) * n, off_out = off_synd + ((m + 255) & ~(size_t)255),
                 off_cnt = off_out + ((n + 255) & ~(size_t)255), total = off_cnt + 64;
    int rc = ensure(h, tmp, total);
    if (rc) return rc;
    unsigned char* b = (unsigned char*)tmp.p;
    HIP_TRY(h, hipMemsetAsync(b, 0, total, call.lane->stream));
    const int cnt[8] = {0, 1, 0, 0, /*osd_list*/ 0, /*rank_out*/ -1, 0, 0};
    HIP_TRY(h, hipMemcpyAsync(b + off_cnt, cnt, sizeof(cnt), hipMemcpyHostToDevice, call.lane->stream));
    OsdParams P{};
    P.m = h->m; P.n = h->n; P.rank = std::min(h->m, h->n);
    P.osd_method = BPOSD_OSD_0; P.osd_order = 0; P.tie_policy = 0;
    P.synd = b + off_synd; P.rp = h->d_rp; P.ci = h->d_ci; P.llr_ws = (const double*)(b + off_llr);
    P.osd_list = (const int*)(b + off_cnt) + 4; P.counters = (int*)(b + off_cnt);
    P.out_osd0 = nullptr; P.out_osdw = b + off_out;
    HIP_TRY(h, hipEventRecord(call.lane->ev_bp, call.lane->stream));
    HIP_TRY(h, hipStreamWaitEvent(call.osd_stream, call.lane->ev_bp, 0));
    rc = launch_osd_large(h, call, P, 1, (int*)(b + off_cnt) + 5);
    if (!rc) {
        int got[8];
        hipError_t e = hipStreamSynchronize(call.osd_stream);
        if (e == hipSuccess) e = hipMemcpy(got, b + off_cnt, sizeof(got), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(h, BPOSD_ERR_HIP, "rank probe failed: %s", hipGetErrorString(e));
        else if (got[5] < 0 || got[5] > std::min(h->m, h->n)) rc = fail(h, BPOSD_ERR_HIP, "rank probe returned %d", got[5]);
        else *rank = got[5];
    }
    return rc;
}

int num_candidates(const bposd_handle* h) {
    const int w = h->cfg.osd_order;
    if (h->cfg.osd_method <= BPOSD_OSD_0 || w == 0) return 0;
    if (h->cfg.osd_method == BPOSD_OSD_E) return (1 << w) - 1;
    return h->kprime + w * (w - 1) / 2;
}
}  // namespace bposd_host

extern "C" {

int bposd_debug_local_layout(const int32_t* indptr, const int32_t* indices, int32_t m, int32_t n, int64_t* out) {
    // host-only: the ownership / position layout the local-edge BP kernel would use for this pcm.
    // out[0] simulated LDS passes, out[1] ideal passes, out[2] positions in uniform groups, out[3] mixed (group, slot) pairs,
    // out[4] positions MP, out[5..13] class sizes, out[14] modelled ds_write_b64 cycles of the bit pass, out[15] their floor
    if (!indptr || !indices || !out) return BPOSD_ERR_INVALID;
    LocalLayout ll;
    if (const int rc = local_layout_for(indptr, indices, m, n, true, ll)) return rc;
    const int MP = ll.MP;
    const local_layout::Graph& g = ll.g;
    const local_layout::Layout& best = ll.best;
    int mixed = 0;
    for (int gq = 0; gq < MP / 64; ++gq)
        for (int b = 0; b < 2; ++b) {
            int code = -1;
            for (int p = 64 * gq; p < 64 * gq + 64; ++p) {
                const int c = best.pos_chk[p];
                if (c < 0) continue;
                const int d = g.rank_of(best.load[2 * c + b], c);
                code = (code < 0 || code == d) ? d : 3;
            }
            mixed += code == 3;
        }
    out[0] = best.passes; out[1] = 4 * (MP / 32); out[2] = best.nfull; out[3] = mixed; out[4] = MP;
    out[14] = best.wcycles; out[15] = 6 * 4 * (MP / 64);
    for (int k = 0; k < 9; ++k) out[5 + k] = 0;
    for (int c = 0; c < m; ++c) {
        int a = g.rank_of(best.load[2 * c], c), b = g.rank_of(best.load[2 * c + 1], c);
        if (a > b) std::swap(a, b);
        out[5 + a * 3 + b]++;
    }
    return BPOSD_OK;
}

int bposd_debug_local_keys(const int32_t* indptr, const int32_t* indices, int32_t m, int32_t n, int32_t* group_key, int32_t* pos_chk, int64_t* info) {
    // host-only: the wave pairing of the local-edge BP kernel's layout.  group_key[MP / 64]: key of every group as the kernel
    // forms it (local_keys.h); pos_chk[MP]: check at a position (-1: padding); info[0..2]: modelled read cycles, write cycles
    // and mixed (group, slot) pairs of the search's layout, info[3..5]: the same after pairing, info[6]: positions MP,
    // info[7]: waves of the two-checks-per-thread kernel (groups w and w + MP / 128) that run the generic loop body
    if (!indptr || !indices || !group_key || !pos_chk || !info) return BPOSD_ERR_INVALID;
    LocalLayout ll;
    if (const int rc = local_layout_for(indptr, indices, m, n, false, ll)) return rc;
    const int MP = ll.MP;
    const local_layout::Graph& g = ll.g;
    local_layout::Layout& best = ll.best;
    local_layout::LdsCost t = local_layout::lds_cost(g, best);
    info[0] = t.read_cycles; info[1] = t.write_cycles; info[2] = t.mixed;
    if (local_layout::pair_groups(g, best) < 0) return BPOSD_ERR_UNSUPPORTED;
    t = local_layout::lds_cost(g, best);
    info[3] = t.read_cycles; info[4] = t.write_cycles; info[5] = t.mixed;
    info[6] = MP; info[7] = best.generic_waves;
    const std::vector<int> keys = local_layout::group_keys(g, best);
    for (int gq = 0; gq < MP / 64; ++gq) group_key[gq] = keys[gq];
    for (int p = 0; p < MP; ++p) pos_chk[p] = best.pos_chk[p];
    return BPOSD_OK;
}

int bposd_debug_local_waves(const int32_t* indptr, const int32_t* indices, int32_t m, int32_t n, int32_t* wave_body, int64_t* info) {
    // host-only: which loop body every wave of the two-checks-per-thread kernels runs (local_layout::wave_plan) and the
    // instance that holds them.  wave_body[MP / 128]: one of the seven group keys, a pair key (local_keys.h), -1 = generic;
    // info[0] positions MP, info[1] PAIRKEY of the instance the host launches (-1: the plain one), info[2] waves on the
    // generic body, info[3] the mode (0 generic, 1 demotion, 2 pair body)
    if (!indptr || !indices || !wave_body || !info) return BPOSD_ERR_INVALID;
    LocalLayout ll;
    if (const int rc = local_layout_for(indptr, indices, m, n, true, ll)) return rc;
    const int MP = ll.MP;
    const local_layout::Graph& g = ll.g;
    const local_layout::Layout& best = ll.best;
    const local_layout::PairMode mode = local_layout::pair_mode();
    const local_layout::WavePlan plan = local_layout::wave_plan(g, best, mode);
    for (int w = 0; w < MP / 128; ++w) wave_body[w] = plan.body[w];
    info[0] = MP; info[1] = plan.pair_key; info[2] = plan.generic; info[3] = (int)mode;
    return BPOSD_OK;
}

int bposd_debug_class_layout(const int32_t* indptr, const int32_t* indices, int32_t m, int32_t n, int32_t* pos_chk, int32_t* pos_bit,
                             int32_t* bit_slot, int32_t* grp_deg, int32_t* grp_cdeg, int64_t* info) {
    // host-only: the tables bp_class_kernel would be launched with for this pcm (tests check their invariants without a GPU).
    // info[0..10]: DC, DVLO, DVHI, VPT, MP (= NTMAX), threads per workgroup, modelled read cycles, their floor, modelled write cycles, their
    // floor, DCLO
    if (!indptr || !indices || !info || m < 1 || n < 1) return BPOSD_ERR_INVALID;
    std::vector<int> rp(indptr, indptr + m + 1), ci(indices, indices + indptr[m]);
    for (int e : ci)
        if (e < 0 || e >= n) return BPOSD_ERR_INVALID;
    const ClassShape* shp = class_shape_for(rp, ci, m, n);
    if (!shp || m > 1024) return BPOSD_ERR_UNSUPPORTED;
    class_layout::Tables T;
    bool ok = false;
    for (int mp : {256, 512, 1024}) {
        if (m > mp) continue;
        if (class_layout::build(rp, ci, m, n, shp->dclo, shp->dc, shp->dvlo, shp->dvhi, kClassVPT, mp, mp, class_layout_iters(), T)) { ok = true; break; }
    }
    if (!ok) return BPOSD_ERR_UNSUPPORTED;
    info[0] = shp->dc; info[1] = shp->dvlo; info[2] = shp->dvhi; info[3] = kClassVPT; info[4] = T.MP; info[5] = T.NT;
    info[6] = T.read_cycles; info[7] = T.read_floor; info[8] = T.write_cycles; info[9] = T.write_floor; info[10] = shp->dclo;
    if (pos_chk) std::copy(T.pos_chk.begin(), T.pos_chk.end(), pos_chk);    // [MP]
    if (pos_bit) std::copy(T.pos_bit.begin(), T.pos_bit.end(), pos_bit);    // [VPT * MP]
    if (bit_slot) std::copy(T.bit_slot.begin(), T.bit_slot.end(), bit_slot);  // [DVHI * VPT * MP]
    if (grp_deg) std::copy(T.grp_deg.begin(), T.grp_deg.end(), grp_deg);    // [VPT * MP / 64]
    if (grp_cdeg) std::copy(T.grp_cdeg.begin(), T.grp_cdeg.end(), grp_cdeg);  // [MP / 64]
    return BPOSD_OK;
}

}  // extern "C"
