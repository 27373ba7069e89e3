"""The whole chain against the oracle at every k-mer size the build stage treats differently, not only at k = 25: a fixed-k
sweep from 13 to 255 on mixed batches (tests/kmer_size_cases.py), ladders that put windows on both sides of a packing
boundary into one launch, the graph / cleaning / hint / lane routes at the boundary sizes, and reads and reference windows
whose length is k - 1, k, k + 1.  Every comparison is the bit-exact one of test_process_batch_seed_sweep (the annotation's
floats within the harness's SEQCX_FLOAT_TOL); every case asserts on the oracle's output that it is not empty."""
import numpy as np
import pytest

import kmer_size_cases as kc
from harness import OracleEngine, compare_asm, compare_cx, compare_geno, compare_vars
from lancet2_amd import capi, synth
from lancet2_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _oracle_chain(params, arrs, n, nr):
    orc = OracleEngine(params)
    wg = orc.gate(arrs, n, nr)
    wa = orc.assemble(arrs, n, nr)
    wv = orc.msa(arrs, n, nr, wa)
    wq = orc.genotype(arrs, n, nr, wa, wv)
    wc = orc.annotate(arrs, n, nr, wa, wv)
    return wg, wa, wv, wq, wc


def _whole_chain_equals(params, arrs, n, nr, want, tag=""):
    wg, wa, wv, wq, wc = want
    eng = Engine(params)
    try:
        g, a, v, q = eng.process(arrs, n, nr, debug=True)
        cx = eng.annotate(arrs, n, nr, a, v)
    finally:
        eng.close()
    assert np.array_equal(g["max_approx"], wg["max_approx"]) and np.array_equal(g["max_exact"], wg["max_exact"]), tag
    bad = compare_asm(params, a, wa, n) + compare_vars(params, v, wv, n)
    bad += compare_geno(params, q, wq, n, nr, wv["win_nvars"], arrs["read_win_off"])
    assert not bad, tag + "\n" + "\n".join(bad[:20])
    compare_cx(params, cx, wc, wv["win_nvars"])


# ---- 1 + 6: fixed-k sweep of the whole chain --------------------------------------------------------------------------

@pytest.mark.parametrize("K", kc.SWEEP_KS + kc.HIGH_KS)
def test_whole_chain_at_fixed_k(K):
    """min_k = max_k = K: every window of a mixed batch (plain, soft clips + N, STR, lower case, noisy, 250-base reads from
    K = 97, a short window) and of a three-sample batch is attempted at exactly K.  The floor (half the windows of a batch
    with a component of >= 2 haplotypes, a variant, win_k == K) is asserted on the oracle before the engine runs.
    K = 129, 191, 255 lie above the default max_k and at the reference's bound (cbdg/graph_params.h:15): 250-base reads,
    1301-base windows."""
    for name, params, arrs, n, nr in kc.sweep_batches(K):
        want = _oracle_chain(params, arrs, n, nr)
        bad = kc.floor_of(K, want[1], want[2], n)[3]
        assert not bad, f"{name}: {bad}"
        _whole_chain_equals(params, arrs, n, nr, want, f"k={K} {name}")


@pytest.mark.parametrize("K", [25, 79, 81, 83])
def test_reads_on_both_sides_of_the_fast_path_mask(K):
    """k_classify's fast path covers reads of at most 320 k-mers; nk = len - k + 1, so a 400-base read has 376 k-mers at
    k = 25, 322 at 79 (generic path), exactly 320 at 81 and 318 at 83 (fast path).  Four windows of such reads (one with N and
    soft clips) beside two windows of 150-base reads, the whole chain."""
    params = kc.sweep_params(K)
    f = 140_000 + 100 * K
    long_kw = dict(synth.CONFIGS["C2"], read_len=400)
    wins = [synth.make_window(f + 0, **long_kw), synth.make_window(f + 1, **synth.CONFIGS["C2"]),
            synth.make_window(f + 2, softclip_frac=0.08, n_frac=0.05, **long_kw), synth.make_window(f + 3, **long_kw),
            synth.make_window(f + 4, **synth.CONFIGS["C3"]), synth.make_window(f + 5, **long_kw)]
    arrs, n, nr = synth.pack_batch(wins)
    assert int(np.diff(arrs["read_off"]).max()) - K + 1 == 401 - K
    want = _oracle_chain(params, arrs, n, nr)
    bad = kc.floor_of(K, want[1], want[2], n)[3]
    assert not bad, bad
    _whole_chain_equals(params, arrs, n, nr, want, f"k={K}")


# ---- 3: ladders that straddle a boundary inside one launch ---------------------------------------------------------------

def _ladder_windows(first, dups, **over):
    wins = []
    for i, dup in enumerate(dups):
        kw = dict(synth.CONFIGS["C2"], **over)
        if dup:
            kw["tandem_dup"] = dup
        wins.append(synth.make_window(first + i, **kw))
    return synth.pack_batch(wins)


LADDERS = [
    # (min_k, max_k, k_step), tandem duplications (0 = none), the boundary the rungs straddle (None: just two distinct rungs)
    ((31, 33, 2), (0, 31, 0, 32, 31, 0, 32, 31), 32),
    ((29, 35, 6), (0, 30, 0, 32, 31, 0, 33, 29), 32),
    ((63, 65, 2), (0, 63, 0, 64, 63, 0, 64, 63), 64),
    ((95, 97, 2), (0, 95, 0, 96, 95, 0, 96, 95), 96),
    ((13, 127, 6), (0, 30, 45, 0, 64, 70, 80, 110), None),
]


@pytest.mark.parametrize("ladder,dups,boundary", LADDERS, ids=["-".join(map(str, x[0])) for x in LADDERS])
def test_ladders_that_straddle_a_packing_boundary(ladder, dups, boundary, monkeypatch):
    """Windows that assemble at the first rung beside windows whose tandem duplication (as long as the first rung or longer)
    sends them up: one launch holds windows at k <= 32 and k > 32 (or <= 64 and > 64, <= 96 and > 96).  The whole chain, with
    the six-rungs tail on and off; the default ladder with duplications up to 110 bases too."""
    params = capi.default_params(min_k=ladder[0], max_k=ladder[1], k_step=ladder[2])
    over = dict(depths=(45, 45)) if ladder[0] >= 95 else {}
    arrs, n, nr = _ladder_windows(120_000 + 10 * ladder[0], dups, **over)
    want = _oracle_chain(params, arrs, n, nr)
    ks = set(want[1]["win_k"][want[1]["win_ncomp"] > 0].tolist())
    assert len(ks) >= 2, want[1]["win_k"].tolist()
    if boundary is not None:
        assert min(ks) <= boundary < max(ks), sorted(ks)
    else:
        assert max(ks) > 64 and min(ks) <= 31, sorted(ks)
    assert int(want[2]["win_nvars"].sum()) >= 1
    for no_spec in (False, True):
        if no_spec:
            monkeypatch.setenv("MA_NO_SPEC", "1")
        else:
            monkeypatch.delenv("MA_NO_SPEC", raising=False)
        _whole_chain_equals(params, arrs, n, nr, want, f"ladder {ladder} MA_NO_SPEC={int(no_spec)}")


# ---- 4: route crosses at the boundary sizes ------------------------------------------------------------------------------

def _assemble(params, arrs, n, nr, streams=None):
    eng = Engine(params)
    try:
        if streams is not None:
            eng.set_streams(streams)
        eng.timing_control(1)
        a = eng.assemble(arrs, n, nr)
        return a, {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()


@pytest.mark.parametrize("K", kc.ROUTE_KS)
def test_routes_at_the_boundary_sizes(K, monkeypatch):
    """The general graph kernels (MA_NO_GRAPH_FUSE), cleaning from the raw graph (MA_NO_CHAINS), absent / shifted / random
    read hints and two lanes, on the sweep's mixed batch at k = 31, 33, 65, 127: the oracle's assembly every time."""
    for key in ("MA_NO_GRAPH_FUSE", "MA_NO_CHAINS"):
        monkeypatch.delenv(key, raising=False)
    _name, params, arrs, n, nr = kc.sweep_batches(K)[0]
    want = OracleEngine(params).assemble(arrs, n, nr)
    assert not kc.floor_of(K, want, None, n)[3]

    def check(tag, a):
        bad = compare_asm(params, a, want, n)
        assert not bad, f"k={K} {tag}: " + "\n".join(bad[:10])

    a, names = _assemble(params, arrs, n, nr)
    assert "k_graph" in names, sorted(names)
    assert "k_clean_chains" in names, sorted(names)
    check("default", a)
    monkeypatch.setenv("MA_NO_GRAPH_FUSE", "1")
    a, names = _assemble(params, arrs, n, nr)
    assert "k_graph" not in names and "k_graph_gen" in names, sorted(names)
    check("MA_NO_GRAPH_FUSE", a)
    monkeypatch.delenv("MA_NO_GRAPH_FUSE")
    monkeypatch.setenv("MA_NO_CHAINS", "1")
    a, names = _assemble(params, arrs, n, nr)
    assert "k_clean_chains" not in names, sorted(names)
    check("MA_NO_CHAINS", a)
    monkeypatch.delenv("MA_NO_CHAINS")
    a, _ = _assemble(params, arrs, n, nr, streams=2)
    check("two lanes", a)
    rng = np.random.default_rng(K)
    hints = {
        "none": None,
        "no_hint_value": np.full(nr, capi.MA_NO_HINT, dtype=np.int32),
        "shifted": (arrs["read_hint"] + rng.integers(-3, 4, nr)).astype(np.int32),
        "random": rng.integers(-400, 1400, nr).astype(np.int32),
    }
    eng = Engine(params)
    try:
        for name, h in hints.items():
            a2 = dict(arrs)
            if h is None:
                a2.pop("read_hint")
            else:
                a2["read_hint"] = h
            check("hints " + name, eng.assemble(a2, n, nr))
    finally:
        eng.close()


# ---- 5: lengths around k ---------------------------------------------------------------------------------------------------

def _read(seq, qname, sample=0, role=0, start=0):
    seq = np.frombuffer(seq, np.uint8).copy() if isinstance(seq, bytes) else np.asarray(seq, np.uint8).copy()
    return dict(seq=seq, qual=np.full(len(seq), 35, np.uint8), qname=qname, sample=sample, role=role, rev=False, passf=True,
                start=start, hint=start)


def _with_extra_reads(win, extra):
    reads = list(win["reads"]) + extra
    reads.sort(key=lambda r: (0 if r["passf"] else 1, r["role"], r["sample"], r["qname"], r["start"]))
    return dict(ref=win["ref"], reads=reads)


def _short_reads_of(ref, lens, qname0, n_every=0):
    """reads cut out of the reference with the given lengths, cycling; n_every > 0: an N at every n_every-th base"""
    out = []
    for i, ln in enumerate(lens):
        if ln <= 0 or ln > len(ref):
            continue
        at = (37 * i) % (len(ref) - ln + 1)
        seq = ref[at:at + ln].copy()
        if n_every:
            seq[n_every - 1::n_every] = ord("N")
        out.append(_read(seq, qname0 + i, sample=i & 1, role=i & 1, start=at))
    return out


@pytest.mark.parametrize("K", [25, 33, 127])
def test_lengths_around_k(K):
    """Reads of K - 1, K, K + 1 and K + 2 bases (a read of exactly K bases has one k-mer, a shorter one none), a read that is
    all N, a read with an N every K - 1 bases (no valid k-mer), reference windows of K - 1, K, K + 1 and min_anchor_len + K
    bases, and a window whose only reads are shorter than K -- mixed into a batch with ordinary windows: the oracle's statuses
    and results in every window, the neighbours' included."""
    params = kc.sweep_params(K)
    f = 130_000 + 100 * K
    kw = dict(synth.CONFIGS["C2"])
    if K >= 111:
        kw["depths"] = (60, 60)
    plain = [synth.make_window(f + i, **kw) for i in range(4)]
    ref0 = plain[0]["ref"]
    rng = np.random.default_rng(f)
    odd = _short_reads_of(ref0, [K - 1, K, K + 1, K + 2] * 6, 900_000)
    odd += [_read(np.full(150, ord("N"), np.uint8), 900_100 + i, sample=i & 1, role=i & 1, start=100 * i) for i in range(3)]
    odd += _short_reads_of(ref0, [150, 150, 2 * K, 149], 900_200, n_every=K - 1)
    wins = [_with_extra_reads(plain[0], odd), plain[1]]
    for j, wl in enumerate((K - 1, K, K + 1, params.min_anchor_len + K)):
        src = synth.make_window(f + 10 + j, **dict(kw, W=max(wl, 200)))
        ref = src["ref"][:wl].copy()
        reads = [r for r in src["reads"] if r["start"] + len(r["seq"]) > 0 and r["start"] < wl] if wl > 200 else \
            _short_reads_of(src["ref"], [150] * 40, 910_000 + 100 * j)
        wins.append(dict(ref=ref, reads=reads))
        if j == 1:
            wins.append(plain[2])
    only_short = _short_reads_of(plain[3]["ref"], list(rng.integers(1, K, 60)), 920_000)
    wins.append(dict(ref=plain[3]["ref"].copy(), reads=sorted(only_short, key=lambda r: (r["role"], r["sample"], r["qname"]))))
    wins.append(dict(ref=plain[3]["ref"].copy(), reads=[]))
    wins.append(plain[3])
    arrs, n, nr = synth.pack_batch(wins)
    orc = OracleEngine(params)
    want = orc.assemble(arrs, n, nr)
    ordinary = [0, 1, 4, n - 1]
    MC = params.max_comps
    multi = [int(want["comp_nhaps"][w * MC:(w + 1) * MC].max()) >= 2 for w in ordinary]
    assert sum(multi) >= 2 and (want["win_ncomp"] == 0).sum() >= 5, (multi, want["win_ncomp"].tolist())
    alone = OracleEngine(params).assemble(*synth.pack_batch([plain[1], plain[2], plain[3]]))
    for i, w in enumerate((1, 4, n - 1)):  # the oracle's neighbours do not depend on the batch either
        assert want["win_ncomp"][w] == alone["win_ncomp"][i] and want["win_status"][w] == alone["win_status"][i]
    eng = Engine(params)
    try:
        got = eng.assemble(arrs, n, nr)
    finally:
        eng.close()
    assert np.array_equal(got["win_status"], want["win_status"]), (got["win_status"].tolist(), want["win_status"].tolist())
    bad = compare_asm(params, got, want, n)
    assert not bad, f"k={K}: " + "\n".join(bad[:10])
