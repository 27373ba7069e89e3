"""k_support's group loop against the oracle, bit for bit, on the smallest shapes at which its two routes can differ: the fast
route (cached records, one or two mates of at most 128 k-mers each, everything about the group in scalar registers, one
reservation per queue and group) and the general loop (everything else).  Ordinary synthetic windows carry hand-made groups of
reads cut out of the reference: lengths on both sides of the 64- and 128-k-mer trip boundaries, mates that overlap fully, by
one k-mer, by one base and across the 64-k-mer boundary, a second mate left of the first, a lone mate, three reads of one name,
one name in two separate runs, N and low-quality bases in both mates -- through the default (dedup) queue route, the plain
queue route (MA_NO_GRAPH_FUSE), without hints, with a table retry pass (MA_TC_FIRST), uncached (a window of more than 2048
reads in the batch), with three samples and on a two-rung ladder.  Every case asserts on the oracle's output first that at
least half its ordinary windows have a component of >= 2 haplotypes."""
import numpy as np
import pytest

from harness import OracleEngine, compare_asm
from lancet2_amd import capi, synth
from lancet2_amd.engine import Engine

pytestmark = pytest.mark.gpu

K = 25
W = 600  # synth.CONFIGS["C1"]


def _read(ref, at, ln, qname, sample, role, passf=True, qual=35):
    seq = ref[at:at + ln].copy()
    assert len(seq) == ln, (at, ln, len(ref))
    return dict(seq=seq, qual=np.full(ln, qual, np.uint8), qname=qname, sample=sample, role=role, rev=False, passf=passf,
                start=at, hint=at)


def _group(ref, qname, mates, sample=0, role=0):
    """reads of one (qname, role, sample) in the order given: mates = [(start, length)] or [(start, length, passf)]"""
    return [_read(ref, m[0], m[1], qname, sample, role, *(m[2:3])) for m in mates]


def _with_groups(win, groups, tail=()):
    """the window's own reads and the hand-made groups in collector order (pass first, role, sample, qname; the order inside a
    hand-made group as given), then `tail` appended as it is (a name's second, separate run)"""
    reads = list(win["reads"]) + [r for g in groups for r in g]
    reads.sort(key=lambda r: (0 if r["passf"] else 1, r["role"], r["sample"], r["qname"]))  # (stable)
    return dict(ref=win["ref"], reads=reads + list(tail))


def _c1(index, **kw):
    return synth.make_window(index, **dict(synth.CONFIGS["C1"], **kw))


def _boundary_window(index, sample, role):
    """63 / 64 / 65 and 127 / 128 / 129 k-mers; unequal mates; fast groups right before and after groups that fall back"""
    win = _c1(index)
    ref, q = win["ref"], 800_000
    lens = [(87, 87), (88, 152), (88, 153), (89, 151), (152, 152), (153, 153), (88, 88), (153, 88), (151, 89), (152, 87)]
    groups = [_group(ref, q + i, [(20 + 31 * i, la), (60 + 37 * i, lb)], sample, role) for i, (la, lb) in enumerate(lens)]
    return _with_groups(win, groups)


def _overlap_window(index, sample, role):
    """the second mate against the first mate's counted offsets: o0 = 0 (full overlap), 63, 64, 127 (one k-mer shared), 128
    (bases overlap, no k-mer shared), 151 (one base), negative (second mate left of the first), beyond the first mate"""
    win = _c1(index)
    ref, q, s = win["ref"], 810_000, 100
    groups = [_group(ref, q + i, [(s, 152), (s + d, ln)], sample, role)
              for i, (d, ln) in enumerate([(0, 152), (63, 152), (64, 152), (127, 152), (128, 152), (151, 152), (0, 88), (63, 88),
                                           (64, 89), (126, 150), (300, 150)])]
    groups += [_group(ref, q + 50 + i, [(s + d, 150), (s, 152)], sample, role) for i, d in enumerate([1, 40, 63, 64, 127, 130])]
    groups += [_group(ref, q + 60, [(s + 40, 88), (s, 87)], sample, role)]
    return _with_groups(win, groups)


def _shape_window(index, sample, role):
    """a lone mate (the other one filtered), three and four reads of one (qname, role), a read shorter than k beside its mate,
    N and low-quality bases in both mates"""
    win = _c1(index, n_frac=0.2, softclip_frac=0.1)
    ref, q = win["ref"], 820_000
    groups = [_group(ref, q + 0, [(50, 150, True), (200, 150, False)], sample, role),
              _group(ref, q + 1, [(80, 150, False), (130, 150, True)], sample, role),
              _group(ref, q + 2, [(30, 150), (90, 150), (150, 150)], sample, role),
              _group(ref, q + 3, [(300, 150), (310, 120)], sample, role),
              _group(ref, q + 4, [(10, 88), (40, 152), (70, 88), (100, 152)], sample, role),
              _group(ref, q + 5, [(400, 150), (420, 24)], sample, role),
              _group(ref, q + 6, [(410, 24), (380, 150)], sample, role)]
    for i, (a, b) in enumerate([(200, 260), (330, 330), (120, 60)]):
        g = _group(ref, q + 10 + i, [(a, 150), (b, 152)], sample, role)
        for r, at in zip(g, (30 + 40 * i, 63 + i)):
            r["seq"][at] = ord("N")
            r["qual"][at] = 2
            r["qual"][100:112] = 5  # (low-quality bases: k-mers over them are not error free)
            r["seq"][105] = ord("ACGT"[(b"ACGT".index(bytes([r["seq"][105]])) + 1) % 4])
        groups.append(g)
    return _with_groups(win, groups)


def _two_runs_window(index):
    """one (qname, role) in two separate runs of adjacent reads: check (X) sends every group of the window down the general set"""
    win = _c1(index)
    ref = win["ref"]
    groups = [_group(ref, 830_000, [(40, 150), (120, 152)], 1, 1), _group(ref, 830_001, [(200, 88), (210, 152)], 1, 1)]
    return _with_groups(win, groups, tail=_group(ref, 830_000, [(260, 150)], 1, 1))


def _main_windows(f):
    return [_boundary_window(f + 0, 0, 0), _overlap_window(f + 1, 1, 1), _shape_window(f + 2, 1, 1), _c1(f + 3),
            _two_runs_window(f + 4), _boundary_window(f + 5, 1, 1), _overlap_window(f + 6, 0, 0), _shape_window(f + 7, 0, 0)]


def _floor(params, want, ordinary):
    MC = params.max_comps
    multi = [int(want["comp_nhaps"][w * MC:(w + 1) * MC].max()) >= 2 for w in ordinary]
    assert 2 * sum(multi) >= len(ordinary), (multi, want["win_ncomp"].tolist())


def _assemble(params, arrs, n, nr):
    eng = Engine(params)
    try:
        return eng.assemble(arrs, n, nr)
    finally:
        eng.close()


_MAIN = {}


def _main_case():
    """the main batch and the oracle's assembly of it, computed once and left unchanged"""
    if not _MAIN:
        params = capi.default_params(min_k=K, max_k=K)
        arrs, n, nr = synth.pack_batch(_main_windows(150_000))
        lens = np.diff(arrs["read_off"]).astype(np.int64)
        assert {87, 88, 89, 151, 152, 153} <= set(lens.tolist()) and int(np.diff(arrs["read_win_off"]).max()) + 2 <= 2048
        want = OracleEngine(params).assemble(arrs, n, nr)
        _floor(params, want, range(n))
        _MAIN.update(params=params, arrs=arrs, n=n, nr=nr, want=want)
    return _MAIN["params"], _MAIN["arrs"], _MAIN["n"], _MAIN["nr"], _MAIN["want"]


def _check(params, got, want, n, tag):
    assert np.array_equal(got["win_status"], want["win_status"]), (tag, got["win_status"].tolist(), want["win_status"].tolist())
    bad = compare_asm(params, got, want, n)
    assert not bad, tag + "\n" + "\n".join(bad[:20])


_ENV_KEYS = ("MA_NO_GRAPH_FUSE", "MA_TC_FIRST", "MA_NO_CAP_RETRY")


@pytest.mark.parametrize("env", [{}, {"MA_NO_GRAPH_FUSE": "1"}, {"MA_TC_FIRST": "10"}, {"MA_NO_GRAPH_FUSE": "1", "MA_TC_FIRST": "10"}],
                         ids=["dedup", "plain_queue", "table_retry", "plain_queue_table_retry"])
def test_group_shapes_on_every_queue_route(env, monkeypatch):
    """Trip boundaries, unequal mates, overlaps at offsets 0 / 63 / 64 / 127 / 128, a second mate left of the first, lone mates,
    runs of three and four, N and low-quality bases, one name in two runs: the counts queued for k_graph (dedup mode, the
    default), the keys queued for k_mm_q (MA_NO_GRAPH_FUSE), and both again when the first table is planned too small and the
    retry pass sends the mate-mers through the HBM set (MA_TC_FIRST=10)."""
    for key in _ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    params, arrs, n, nr, want = _main_case()
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    got = _assemble(params, arrs, n, nr)
    assert not (got["win_status"] & capi.MA_W_TABLE_OVERFLOW).any()
    _check(params, got, want, n, str(env))


@pytest.mark.parametrize("hints", ["absent", "no_hint_value", "every_third"])
def test_group_shapes_without_hints(hints, monkeypatch):
    """No read_hint array and every hint MA_NO_HINT: every group is generic and the general instances are flagged in their
    words (kInstGen) for the set kernels; a third of the reads without a hint: generic groups between ordinary ones."""
    for key in _ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    params, arrs, n, nr, want = _main_case()
    a2 = dict(arrs)
    if hints == "absent":
        a2.pop("read_hint")
    elif hints == "no_hint_value":
        a2["read_hint"] = np.full(nr, capi.MA_NO_HINT, dtype=np.int32)
    else:
        h = arrs["read_hint"].copy()
        h[::3] = capi.MA_NO_HINT
        a2["read_hint"] = h
    _check(params, _assemble(params, a2, n, nr), want, n, hints)


def test_uncached_window_beside_ordinary_ones(monkeypatch):
    """A window of more than 2048 reads: the records of no window of the launch are cached, the set-up passes read the batch's
    arrays and every group takes the general loop -- the hand-made groups included."""
    for key in _ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    params = capi.default_params(min_k=K, max_k=K)
    deep = _c1(151_000, depths=(260, 260))
    wins = [_boundary_window(151_001, 0, 0), deep, _overlap_window(151_002, 1, 1), _shape_window(151_003, 0, 0)]
    arrs, n, nr = synth.pack_batch(wins)
    assert len(deep["reads"]) > 2048
    want = OracleEngine(params).assemble(arrs, n, nr)
    _floor(params, want, [0, 2, 3])
    _check(params, _assemble(params, arrs, n, nr), want, n, "uncached")


def test_three_samples(monkeypatch):
    """num_samples = 3: an odd counter stride (five packed 16-bit counters per reference position), hand-made groups in each
    sample"""
    for key in _ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    params = capi.default_params(min_k=K, max_k=K, num_samples=3)
    c5 = dict(synth.CONFIGS["C5"], W=W)
    wins = []
    for i, (sample, role) in enumerate([(0, 0), (1, 0), (2, 1), (2, 1)]):
        base = synth.make_window(152_000 + i, **c5)
        src = (_boundary_window, _overlap_window, _shape_window, _boundary_window)[i](152_100 + i, sample, role)
        extra = [r for r in src["reads"] if r["qname"] >= 800_000]
        moved = [dict(r, seq=base["ref"][r["start"]:r["start"] + len(r["seq"])].copy()) for r in extra]
        for r, m in zip(extra, moved):  # (keep the N the shape window planted)
            m["seq"][r["seq"] == ord("N")] = ord("N")
        wins.append(_with_groups(base, [moved]))
    arrs, n, nr = synth.pack_batch(wins)
    assert set(arrs["read_sample"].tolist()) == {0, 1, 2}
    want = OracleEngine(params).assemble(arrs, n, nr)
    _floor(params, want, range(n))
    _check(params, _assemble(params, arrs, n, nr), want, n, "three samples")
    monkeypatch.setenv("MA_NO_GRAPH_FUSE", "1")
    _check(params, _assemble(params, arrs, n, nr), want, n, "three samples, plain queue")


def test_two_rung_ladder(monkeypatch):
    """min_k = 25, max_k = 31: windows whose tandem duplication sends them to the second rung beside windows that assemble at
    the first -- one launch of the second pass holds windows at two k (a read of 88 bases has 64 k-mers at 25 and 58 at 31)."""
    for key in _ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    params = capi.default_params(min_k=25, max_k=31, k_step=6)
    wins = []
    for i, dup in enumerate((0, 27, 0, 28, 26, 0)):
        base = synth.make_window(153_000 + i, **dict(synth.CONFIGS["C2"], W=W, **({"tandem_dup": dup} if dup else {})))
        src = (_boundary_window, _overlap_window, _shape_window)[i % 3](153_100 + i, i & 1, i & 1)
        moved = [dict(r, seq=base["ref"][r["start"]:r["start"] + len(r["seq"])].copy()) for r in src["reads"] if r["qname"] >= 800_000]
        wins.append(_with_groups(base, [moved]))
    arrs, n, nr = synth.pack_batch(wins)
    want = OracleEngine(params).assemble(arrs, n, nr)
    ks = set(want["win_k"][want["win_ncomp"] > 0].tolist())
    assert ks == {25, 31}, want["win_k"].tolist()
    _floor(params, want, range(n))
    _check(params, _assemble(params, arrs, n, nr), want, n, "ladder 25-31")
