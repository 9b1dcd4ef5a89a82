"""The fp64 candidate sweep of osd_kernel<W> and osd_large_kernel<RPT> at every instance edge against the CPU oracle, with
channels whose candidate weights tie (run with -m gpu on an MI355X).

One case per row of tests/weight_cases.py WEIGHT_EDGES and kind of channel: a two-valued ``channel_probs`` vector, a
two-valued channel of its own per shot (``prior_select`` / ``alt_channel_probs``), the same as ``channel_probs_rows``, rows
all equal to the constructor's uniform channel (the fp64 sweep on weights that tie exactly like Hamming weights), and on the
largest shapes a continuous vector.  Every syndrome lies in the column space of H, so every output and every LLR bit must
equal the oracle's, shot by shot, and no shot is left out; ``last_instance()`` names the instance the row was written for;
a second decode of the batch gives the same outputs.  tests/test_weight_cpu.py asserts on the oracle that these inputs make
the winner depend on the order of the additions and on the tie rule, which a continuous channel never does."""
import numpy as np
import pytest

from tests import weight_cases as wc
from tests.test_gpu_parity import _compare_exact

pytestmark = pytest.mark.gpu

CASES = [(r["id"], k) for r in wc.WEIGHT_EDGES for k in wc.row_kinds(r)]


@pytest.fixture(scope="module")
def gpu_ready():
    from bp_osd_amd import _lib

    lib = _lib.load()  # raises loudly if the HIP extension is missing
    assert lib.bposd_device_count() > 0, "no MI355X visible"
    return lib


def _decode(dec, S, **kw):
    osdw = dec.decode_batch(S, want_osd0=True, want_bp=True, want_llr=True, **kw)
    return dict(osdw=osdw, osd0=dec.batch_osd0, bp=dec.batch_bp, converged=dec.batch_converge, iters=dec.batch_iter, llr=dec.batch_llr)


def _same(a, b):
    assert a.get("llr") is not None and b.get("llr") is not None and len(a["osdw"]) == len(b["osdw"])
    _compare_exact(a, b)


def _decoder(row, **channel):
    from bp_osd_amd import BpOsdDecoder

    g = BpOsdDecoder(wc.matrix(row["edge"]), **wc.settings(row), **channel)
    g.set_osd_variant(row["osd_variant"])
    return g


def _check(g, row, S, ref, **kw):
    """Decode, compare with the oracle, name the instance, decode again."""
    got = _decode(g, S, **kw)
    inst = g.last_instance()
    _same(got, ref)
    assert len(got["osdw"]) == len(S)
    if not ref["converged"].all():  # (the OSD kernel is launched for non-converged shots only)
        assert inst["osd"] == wc.expected_osd(row), inst
    again = _decode(g, S, **kw)
    for k in ("osdw", "osd0", "bp", "converged", "iters"):
        assert (again[k] == got[k]).all(), f"{k} differs between two decodes of the same batch"
    assert (again["llr"].view(np.uint64) == got["llr"].view(np.uint64)).all()
    return got


@pytest.mark.parametrize("row_id,kind", CASES, ids=[f"{r}-{k}" for r, k in CASES])
def test_weighted_sweep_vs_oracle(gpu_ready, row_id, kind):
    row, inp = wc.ROW_BY_ID[row_id], wc.inputs(row_id)
    S = inp["S"]
    ref = wc.reference(row_id, kind)
    assert 2 * int((ref["converged"] == 0).sum()) > len(S), "most shots converged"
    if kind in ("vector", "continuous"):
        _check(_decoder(row, channel_probs=inp["vec"] if kind == "vector" else inp["cont"]), row, S, ref)
        return
    g = _decoder(row, error_rate=inp["q"])
    if kind == "select":
        _check(g, row, S, ref, prior_select=inp["sel"], alt_channel_probs=inp["alt"])
    elif kind == "rows":  # the oracle, and the select call of the same draw in every output and every LLR bit
        got = _check(g, row, S, ref, channel_probs_rows=inp["rows"])
        _same(got, _decode(g, S, prior_select=inp["sel"], alt_channel_probs=inp["alt"]))
    else:  # flat-rows: the oracle's uniform decode, and the handle's own plain (integer-path) call
        got = _check(g, row, S, ref, channel_probs_rows=inp["flat"])
        _same(got, _decode(g, S))


@pytest.mark.parametrize("row_id", wc.UPDATE_ROWS)
def test_update_channel_probs_flips_the_weight_path_both_ways(gpu_ready, row_id):
    """uniform (integer weights), update_channel_probs(two-valued) (fp64 weights; on the HBM path another workspace layout),
    update_channel_probs(uniform) (integer weights again) on one handle, each step against the oracle taken the same way."""
    row, inp = wc.ROW_BY_ID[row_id], wc.inputs(row_id)
    g = _decoder(row, error_rate=inp["q"])
    for channel, ref in zip(wc.update_channels(row_id), wc.update_references(row_id)):
        if channel is not None:
            g.update_channel_probs(channel)
        _check(g, row, inp["S"], ref)
    _same(wc.update_references(row_id)[0], wc.update_references(row_id)[2])  # (the oracle itself is back where it began)


def test_probabilities_of_exactly_one_and_zero(gpu_ready):
    """Three entries of exactly 1.0 (cost 0) and three of exactly 0.0 (cost +inf) on bits that pairwise share no check."""
    row = wc.ROW_BY_ID[wc.EXTREME_ROW]
    vec, _ = wc.extreme_vector()
    ref = wc.reference(wc.EXTREME_ROW, "extreme")
    assert not np.isnan(ref["llr"]).any()
    _check(_decoder(row, channel_probs=vec), row, wc.inputs(wc.EXTREME_ROW)["S"], ref)
