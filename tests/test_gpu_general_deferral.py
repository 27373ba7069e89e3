"""The build stage's common-route-only pass (build.hip: run_build_pass, GraphWs::defer_general) and the per-pass clears that
moved into k_select_active, against the oracle and against the engine under MA_NO_DEFER=1.  In the mode pass 0 launches none
of k_mm_q / k_mm_lds / k_mm_hbm / k_graph_gen; a window that needs one comes back through the capacity retry pass, which shows
as a second k_classify launch.  The mode is for a lane that works beside other lanes (alone on the chip the idle launches cost
nothing worth a second pass), so every case here runs ma_process_batch on TWO lanes: each lane is a context with a chunk of
its own, and the launch counts below are per lane times two.  One case pins that a single lane keeps the full order.
tests/test_general_deferral_inputs.py checks the inputs (tests/deferral_cases.py) on the CPU.

k_graph's hand-back (a full edge set, l_fail) has no input among the suite's shapes that reaches it; the branch sets the same
two bits as the kernel's early return, which the mixed batch does reach when a window's table outgrows k_graph's."""
import numpy as np
import pytest

import deferral_cases as dc
from harness import OracleEngine, compare_asm, compare_geno_calls, compare_vars
from lancet2_amd import capi, synth
from lancet2_amd.engine import Engine

pytestmark = pytest.mark.gpu

GENERAL = ("k_mm_q", "k_mm_lds", "k_mm_hbm", "k_graph_gen")
_ENV = ("MA_NO_DEFER", "MA_NO_GRAPH_FUSE", "MA_TC_FIRST", "MA_NO_CAP_RETRY", "MA_NO_SPEC", "MA_STREAMS", "MA_NO_CHAINS")
_CACHE = {}


def _clean_env(monkeypatch):
    for key in _ENV:
        monkeypatch.delenv(key, raising=False)


def _case(name, wins_fn, params):
    """a packed batch and the oracle's outputs of the whole chain, computed once and left unchanged"""
    if name not in _CACHE:
        wins = wins_fn()
        arrs, n, nr = synth.pack_batch(wins)
        orc = OracleEngine(params)
        wa = orc.assemble(arrs, n, nr)
        wv = orc.msa(arrs, n, nr, wa)
        wq = orc.genotype(arrs, n, nr, wa, wv, debug=False)
        _CACHE[name] = (arrs, n, nr, wa, wv, wq)
    return _CACHE[name]


def _count(times, name):
    return sum(1 for k, _ in times if k == name)


def _process(eng, arrs, n, nr):
    eng.timing_control(2)  # (one entry per launch, from this call on)
    g, a, v, q = eng.process(arrs, n, nr)
    return (a, v, q), eng.kernel_times(), eng.stats()


LANES = 2


def _run(params, arrs, n, nr, lanes=LANES):
    eng = Engine(params)
    try:
        eng.set_streams(lanes)
        return _process(eng, arrs, n, nr)
    finally:
        eng.close()


def _same(x, y, tag):
    for got, want in zip(x, y):
        assert got.keys() == want.keys()
        for key in got:
            assert np.array_equal(got[key], want[key], equal_nan=got[key].dtype.kind == "f"), (tag, key)


def _against_oracle(params, out, case, tag):
    arrs, n, nr, wa, wv, wq = case
    a, v, q = out
    assert np.array_equal(a["win_status"], wa["win_status"]), (tag, a["win_status"].tolist(), wa["win_status"].tolist())
    assert np.array_equal(a["win_k"], wa["win_k"]), (tag, a["win_k"].tolist(), wa["win_k"].tolist())
    bad = compare_asm(params, a, wa, n) + compare_vars(params, v, wv, n) + compare_geno_calls(q, wq)
    assert not bad, tag + "\n" + "\n".join(bad[:20])
    assert not (a["win_status"] & capi.MA_W_TABLE_OVERFLOW).any(), tag


def test_headline_shape_nothing_rerouted(monkeypatch):
    """64 of the benchmark's C3 windows at k = 25 on two lanes: every window takes the common route, so no pass launches a
    general kernel and no retry pass follows (one k_classify launch per chunk: a chunk and a pass per lane)."""
    _clean_env(monkeypatch)
    params = capi.default_params(min_k=25, max_k=25)
    case = _case("headline", lambda: dc.headline_windows(64), params)
    out, times, st = _run(params, *case[:3])
    _against_oracle(params, out, case, "headline")
    names = {k for k, _ in times}
    assert not names & set(GENERAL), sorted(names)
    assert _count(times, "k_classify") == LANES and _count(times, "k_graph") == LANES, [k for k, _ in times]


def _rerouted_case(monkeypatch, name, wins_fn):
    """default against MA_NO_DEFER=1 and the oracle; the default run re-assembles the windows that need a general kernel"""
    _clean_env(monkeypatch)
    params = capi.default_params(min_k=25, max_k=25)
    case = _case(name, wins_fn, params)
    out, times, st = _run(params, *case[:3])
    _against_oracle(params, out, case, name)
    # per lane: pass 0 without the general kernels, then the retry pass with them -- each of its kernels once
    assert _count(times, "k_classify") == 2 * LANES, [k for k, _ in times]
    assert _count(times, "k_graph_gen") == LANES and _count(times, "k_mm_q") == LANES and _count(times, "k_mm_hbm") == LANES, \
        [k for k, _ in times]
    monkeypatch.setenv("MA_NO_DEFER", "1")
    out2, times2, st2 = _run(params, *case[:3])
    _same(out, out2, name)
    assert _count(times2, "k_classify") == LANES and _count(times2, "k_graph_gen") == LANES, [k for k, _ in times2]
    assert st["window_attempts"] > st2["window_attempts"], (st, st2)  # every attempt made is counted


def test_mixed_batch_a_few_rerouted(monkeypatch):
    """Sixteen hinted windows, three of them with ~16 k distinct 25-mers (one in the first lane's half, two in the second's):
    their tables outgrow k_insert's map and k_graph, their read support waits for k_mm_q."""
    _rerouted_case(monkeypatch, "mixed", dc.mixed_windows)


def test_mate_mer_support_through_a_general_kernel(monkeypatch):
    """Small windows whose (qname, role) keys come in two separate runs (one such window per lane): every group of such a
    window is generic, and outside queue mode its support goes through the LDS or HBM mate-mer set."""
    _rerouted_case(monkeypatch, "support_groups", lambda: dc.support_group_windows()[0])


def test_single_lane_keeps_the_full_order(monkeypatch):
    """One lane has the chip to itself: the general kernels' idle launches cost nothing there, so the mode stays off -- one
    pass, every kernel of it -- and the outputs are those of two lanes."""
    _clean_env(monkeypatch)
    params = capi.default_params(min_k=25, max_k=25)
    case = _case("mixed", dc.mixed_windows, params)
    out, times, st = _run(params, *case[:3], lanes=1)
    _against_oracle(params, out, case, "one lane")
    assert _count(times, "k_classify") == 1 and _count(times, "k_graph_gen") == 1 and _count(times, "k_mm_q") == 1, [k for k, _ in times]
    out2, _, _ = _run(params, *case[:3])
    _same(out, out2, "one lane against two")


@pytest.mark.parametrize("spec", ["speculative_tail", "rung_by_rung"])
def test_ladder(spec, monkeypatch):
    """k = 13 ... 127, eight windows of which five climb past rung 61 with tables beyond the map.  With the speculative tail
    (default) the upper rungs run in nested passes, which keep the full order; rung by rung (MA_NO_SPEC=1) they are ordinary
    passes of pass 0 and re-route their windows."""
    _clean_env(monkeypatch)
    params = capi.default_params(min_k=13, max_k=127)
    case = _case("ladder", dc.ladder_windows, params)
    assert len(set(case[3]["win_k"].tolist())) >= 3, case[3]["win_k"].tolist()
    if spec == "rung_by_rung":
        monkeypatch.setenv("MA_NO_SPEC", "1")
    out, times, st = _run(params, *case[:3])
    _against_oracle(params, out, case, spec)
    monkeypatch.setenv("MA_NO_DEFER", "1")
    out2, times2, st2 = _run(params, *case[:3])
    _same(out, out2, spec)
    print(spec, "window_attempts", st["window_attempts"], "without the mode", st2["window_attempts"])
    if spec == "rung_by_rung":
        assert st["window_attempts"] > st2["window_attempts"], (st, st2)


def test_context_switches_off(monkeypatch):
    """More than 1 window in 256 re-routed in each lane: the second call on the same engine runs the full order in pass 0 -- one
    k_classify launch per lane, the general kernels present -- and returns what the first call returned."""
    _clean_env(monkeypatch)
    params = capi.default_params(min_k=25, max_k=25)
    case = _case("mixed", dc.mixed_windows, params)
    eng = Engine(params)
    try:
        eng.set_streams(LANES)
        out1, t1, _ = _process(eng, *case[:3])
        out2, t2, _ = _process(eng, *case[:3])
    finally:
        eng.close()
    assert _count(t1, "k_classify") == 2 * LANES and _count(t1, "k_graph_gen") == LANES, [k for k, _ in t1]
    assert _count(t2, "k_classify") == LANES and _count(t2, "k_graph_gen") == LANES and _count(t2, "k_mm_q") == LANES, [k for k, _ in t2]
    _same(out1, out2, "second call")
    _against_oracle(params, out2, case, "second call")


@pytest.mark.parametrize("lanes", ["MA_STREAMS=1", "default", "two_lanes"])
def test_no_stale_state_between_batches(lanes, monkeypatch):
    """One engine on batch A (16 windows, three re-routed), B (4 smaller windows with fewer reads), G (every window stopped by
    the repeat gate: the POA and genotype stages see no assembled window), then A again: the workspace words that
    k_select_active clears hold another batch's values each time."""
    _clean_env(monkeypatch)
    if lanes == "MA_STREAMS=1":
        monkeypatch.setenv("MA_STREAMS", "1")
    params = capi.default_params(min_k=25, max_k=25)
    case_a = _case("mixed", dc.mixed_windows, params)
    case_b = _case("small", dc.small_windows, params)
    case_g = _case("gated", dc.gated_windows, params)
    assert not (case_g[3]["win_ncomp"] > 0).any()
    fresh, _, _ = _run(params, *case_a[:3])  # (two lanes: batch A re-routes its three large windows)
    eng = Engine(params)
    try:
        if lanes == "two_lanes":
            eng.set_streams(2)
        first, _, _ = _process(eng, *case_a[:3])
        small, _, _ = _process(eng, *case_b[:3])
        gated, _, _ = _process(eng, *case_g[:3])
        third, _, _ = _process(eng, *case_a[:3])
    finally:
        eng.close()
    _same(first, third, lanes)
    _same(first, fresh, lanes)
    _against_oracle(params, third, case_a, lanes)
    _against_oracle(params, small, case_b, lanes + " B")
    _against_oracle(params, gated, case_g, lanes + " G")
