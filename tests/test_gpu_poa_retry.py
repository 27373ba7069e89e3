"""The POA stage's retry passes (ma_set_poa_retry, poa.hip: k_poa_retry_select and the passes behind it) against the oracle, on
the hand-made components of tests/poa_cases.py -- what the first pass flags for a width of its graph -- and of
tests/poa_retry_cases.py -- what the second pass holds at its exact fit and flags one over.  tests/test_poa_retry_cases.py
checks the new table on the CPU.

With the setting on a window whose graph overflowed is called by a second pass (eight edge / aligned-node slots per node, or
four and every node one LDS block holds) and equals the oracle with status 0; a window that pass cannot hold either carries
MA_W_VAR_OVERFLOW alone and is compared by status only; MA_W_LEN_OVERFLOW windows are left out as before.  With the setting
off -- or never set -- the flagged windows are the ones tests/test_gpu_poa_cases.py pins.

Every compared value is an integer, a byte or a status word: no tolerance anywhere."""
import numpy as np
import pytest

import poa_cases as pc
import poa_retry_cases as rc
from harness import compare_asm, compare_geno, compare_vars
from lancet2_amd import capi, synth

pytestmark = pytest.mark.gpu

# What the first pass flags for its graph in the groups of poa_cases (by the cause the kernel marks), on every route.
WIDTH_MARKED = {"degree": {"out_degree_5", "out_degree_6", "in_degree_5", "in_degree_6"}, "ring": {"ring_6"},
                "multi": {"over_between_two_fitting"}}
CAPACITY_MARKED = {"headroom_1k": {"ins_8x60"}}
# ... and what it leaves out for its length (never marked, never retried)
LONG = {"length_3072", "length_3073", "length_4096", "length_2552", "narrow_2400_then_17_haplotypes"}
ZERO = {"marked_width": 0, "marked_capacity": 0, "called": 0, "left_flagged": 0}


def _msa(cases, group, retry, route="default", monkeypatch=None, eng=None):
    """one Engine.msa call on a group -> (variant arrays, window status, last_poa_retry()); retry None: the setter is not called"""
    from lancet2_amd.engine import Engine
    for k, v in pc.ROUTES[route].items():
        monkeypatch.setenv(k, v)
    arrs, n, nr, asm = cases.build(group)
    own = eng is None
    if own:
        eng = Engine(cases.groups()[group].params)
    try:
        if retry is not None:
            eng.set_poa_retry(retry)
        got = eng.msa(arrs, n, nr, asm)  # (raises on a return code other than MA_OK)
        counts = eng.last_poa_retry()
    finally:
        if own:
            eng.close()
    return got, asm["win_status"], counts


def _check(cases, group, got, status, flagged_want, route="default"):
    """every window outside flagged_want {name: status bit} equals the oracle with status 0; the others carry exactly their bit
    and are compared by status only (a MA_W_LEN_OVERFLOW window has no variant)"""
    g = cases.groups()[group]
    n = len(g.windows)
    want, want_status = cases.oracle_msa(group)
    masked = {k: np.array(v, copy=True) for k, v in got.items()}
    for wi, w in enumerate(g.windows):
        st = int(status[wi])
        print(f"{group}/{route}: {w.name:30s} status {st:3d} variants {int(got['win_nvars'][wi]):3d} (oracle {int(want['win_nvars'][wi])})")
        if w.name in flagged_want:
            assert st == flagged_want[w.name], (w.name, st)
            if st == capi.MA_W_LEN_OVERFLOW:
                assert int(got["win_nvars"][wi]) == 0, w.name
            for k in masked:
                stride = len(masked[k]) // n
                masked[k][wi * stride:(wi + 1) * stride] = want[k][wi * stride:(wi + 1) * stride]
        else:
            assert st == int(want_status[wi]) == 0, (w.name, st)
    bad = compare_vars(g.params, masked, want, n)
    assert not bad, "\n".join(bad[:20])


def _marks(group):
    nw, nc = len(WIDTH_MARKED.get(group, ())), len(CAPACITY_MARKED.get(group, ()))
    return {"marked_width": nw, "marked_capacity": nc, "called": nw + nc, "left_flagged": 0}


@pytest.mark.parametrize("group", ["degree", "ring", "headroom_1k", "headroom_2400", "multi"])
def test_flagged_windows_of_the_first_pass_are_called(group, monkeypatch):
    """setting on: out_degree_5/6, in_degree_5/6, ring_6, ins_8x60 (in both groups) and over_between_two_fitting -- all three
    components -- equal the oracle with status 0, like every other window; the counts are the marks the table predicts, none
    is left flagged.  (Fails without the retry passes: the seven windows stay MA_W_VAR_OVERFLOW.)"""
    got, status, counts = _msa(pc, group, 1, monkeypatch=monkeypatch)
    _check(pc, group, got, status, {})
    assert counts == _marks(group), counts


@pytest.mark.parametrize("group", ["length", "length_edge", "wide_long"])
def test_windows_left_out_for_their_length_stay_left_out(group, monkeypatch):
    """setting on: the MA_W_LEN_OVERFLOW windows are flagged exactly as with it off, with win_nvars 0, their neighbours equal the
    oracle, and no mark is counted"""
    got, status, counts = _msa(pc, group, 1, monkeypatch=monkeypatch)
    names = {w.name for w in pc.groups()[group].windows}
    _check(pc, group, got, status, {k: capi.MA_W_LEN_OVERFLOW for k in LONG & names})
    assert LONG & names and counts == ZERO, counts


@pytest.mark.parametrize("group", tuple(rc.MARKS))
def test_exact_fit_and_one_over_of_the_second_pass(group, monkeypatch):
    """setting on, the groups of poa_retry_cases: eight edges / a ring of nine / 720 new nodes / both causes in one window /
    a capped component between two others are called and equal the oracle; nine edges / a ring of ten / 1800 new nodes carry
    MA_W_VAR_OVERFLOW alone, their neighbours equal the oracle, the call returns MA_OK, and left_flagged counts them"""
    got, status, counts = _msa(rc, group, 1, monkeypatch=monkeypatch)
    over = {w.name: capi.MA_W_VAR_OVERFLOW for w in rc.groups()[group].windows if w.kind == "over"}
    _check(rc, group, got, status, over)
    nw, nc, left = rc.MARKS[group]
    assert left == len(over)
    assert counts == {"marked_width": nw, "marked_capacity": nc, "called": nw + nc - left, "left_flagged": left}, counts


@pytest.mark.parametrize("group", ["degree", "ring", "headroom_1k"])
@pytest.mark.parametrize("route", [r for r in pc.ROUTES if r != "default"])
def test_first_passes_on_the_other_routes(route, group, monkeypatch):
    """setting on, the first passes as host-counted rounds, with the full fill only, without closed-form alignments, with 32-bit
    label masks for every window (the retry passes then take the LAB32 kernels too) and with the bubble walk's HBM scratch:
    the same results and the same marks.  On the LAB32 route the windows no LAB32 kernel holds stay MA_W_LEN_OVERFLOW, as
    poa_cases.may_flag_on says (none of these three groups has one)"""
    got, status, counts = _msa(pc, group, 1, route, monkeypatch)
    long = {w.name: capi.MA_W_LEN_OVERFLOW for w in pc.groups()[group].windows
            if pc.may_flag_on(route, w) == (True, capi.MA_W_LEN_OVERFLOW)}
    _check(pc, group, got, status, long, route)
    assert counts == _marks(group), counts


@pytest.mark.parametrize("retry", [0, None])
@pytest.mark.parametrize("group", ["degree", "ring", "headroom_1k", "multi"])
def test_setting_off_flags_what_it_flagged_before(group, retry, monkeypatch):
    """setting explicitly off, and a context that never called the setter: the flagged windows are the ones listed here (the
    first pass's widths), everything else equals the oracle, and the counts are all zero"""
    got, status, counts = _msa(pc, group, retry, monkeypatch=monkeypatch)
    flagged = WIDTH_MARKED.get(group, set()) | CAPACITY_MARKED.get(group, set())
    assert flagged
    _check(pc, group, got, status, {k: capi.MA_W_VAR_OVERFLOW for k in flagged})
    assert counts == ZERO, counts


def test_one_context_on_off_on(monkeypatch):
    """one context, three calls on headroom_1k with the setting on, off, on: ins_8x60 is called, flagged, called -- the marks of
    a call do not outlive it and the workspaces are reused"""
    from lancet2_amd.engine import Engine
    eng = Engine(pc.groups()["headroom_1k"].params)
    try:
        for retry in (1, 0, 1):
            got, status, counts = _msa(pc, "headroom_1k", retry, monkeypatch=monkeypatch, eng=eng)
            _check(pc, "headroom_1k", got, status, {} if retry else {"ins_8x60": capi.MA_W_VAR_OVERFLOW})
            assert counts == (_marks("headroom_1k") if retry else ZERO), (retry, counts)
    finally:
        eng.close()


def test_the_setter_takes_0_and_1_only():
    from lancet2_amd.engine import Engine
    eng = Engine(capi.default_params(min_k=25, max_k=25))
    try:
        for bad in (2, -1):
            assert eng.lib.ma_set_poa_retry(eng.h, bad) == -1  # MA_ERR_ARG
        assert eng.lib.ma_set_poa_retry(eng.h, 1) == 0 and eng.lib.ma_set_poa_retry(eng.h, 0) == 0
        assert eng.last_poa_retry() == ZERO
    finally:
        eng.close()


@pytest.mark.parametrize("streams", [1, 2])
def test_the_chained_call_with_the_setting_on(streams):
    """Engine.process on a small synthetic batch, one and two lanes: every output with the setting on equals that with it off,
    no window is marked and the counts are zero.  The hand-made assemblies cannot enter the chain (it assembles its own
    haplotypes from reads), so this checks the plumbing of the setting and of the counts through the lanes, not a retried
    window."""
    from lancet2_amd.engine import Engine
    params = capi.default_params(min_k=25, max_k=25)
    arrs, n, nr = synth.make_config_batch("C1", 6, first_index=900)
    outs = []
    for retry in (0, 1):
        eng = Engine(params)
        try:
            eng.set_streams(streams)
            eng.set_poa_retry(retry)
            outs.append(eng.process(arrs, n, nr, debug=True))
            assert eng.last_poa_retry() == ZERO
        finally:
            eng.close()
    (g0, a0, v0, q0), (g1, a1, v1, q1) = outs
    assert int(v0["win_nvars"].sum()) > 0 and not (a0["win_status"] & capi.MA_W_VAR_OVERFLOW).any()
    assert all(np.array_equal(g0[k], g1[k]) for k in g0)
    bad = compare_asm(params, a1, a0, n) + compare_vars(params, v1, v0, n) + \
        compare_geno(params, q1, q0, n, nr, v0["win_nvars"], arrs["read_win_off"])
    assert not bad, "\n".join(bad[:10])
