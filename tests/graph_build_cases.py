"""The inputs of tests/test_graph_build_ref.py (CPU) and tests/test_gpu_graph_build.py: the synthetic sets of the graph-export
tests, and hand-made windows -- a synthetic three-sample window (roles 0, 0, 1) that assembles, with reads edited so that one
rule of the build or prune stage decides what the pruned graph holds.  Everything here is data; which edge a window reaches is
proved by the counters of tests/graph_build_ref.py, asserted in the CPU file."""
import functools
import types

import numpy as np

from graph_build_ref import PHRED_ERR
from lancet2_amd import capi, synth

K = 25
HM_KW = dict(W=1001, depths=(20, 20, 20), roles=(0, 0, 1))
HM_BASE = dict(mates=3100, gate=3101, labels=3102, singletons=3103, tips=3105, nfilt=3106)  # the windows the edits start from
ROOMY = (512, 2048, 32768)


def _copy(r, **kw):
    c = dict(r)
    c["seq"], c["qual"] = r["seq"].copy(), r["qual"].copy()
    c.update(kw)
    return c


def _offset(read, ctx):
    return bytes(read["seq"]).find(ctx)


def _new_qname(win):
    return max(r["qname"] for r in win["reads"]) + 1


def _other(base, step=1):
    return b"ACGT"[(b"ACGT".index(base) + step) % 4]


def clean_sites(win, left, right, per_sample=4, gap=150):
    """Reference positions p, at least `gap` apart, at which the reads are plain: at least per_sample passing reads of every
    sample hold ref[p - left : p + right] exactly, and they are at least 80 % of the reads that span it."""
    ref, out, p = bytes(win["ref"]), [], 130
    reads = [r for r in win["reads"] if r["passf"]]
    while p < len(ref) - 130:
        ctx = ref[p - left:p + right]
        hits = [r for r in reads if _offset(r, ctx) >= 0]
        cover = [r for r in reads if r["start"] <= p - left - 8 and r["start"] + len(r["seq"]) >= p + right + 8]
        if min(sum(1 for r in hits if r["sample"] == s) for s in range(3)) >= per_sample and len(hits) >= 0.8 * len(cover):
            out.append(p)
            p += gap
        else:
            p += 5
    return out


def holders(win, p, left, right, sample=None):
    """[(read, offset of reference position p in it)] over the passing reads that hold ref[p - left : p + right]"""
    ref = bytes(win["ref"])
    ctx = ref[p - left:p + right]
    out = []
    for r in win["reads"]:
        if r["passf"] and (sample is None or r["sample"] == sample):
            o = _offset(r, ctx)
            if o >= 0:
                out.append((r, o + left))
    return out


def base_window(name):
    return synth.make_window(HM_BASE[name], **HM_KW)


# ---- mate-mers ---------------------------------------------------------------------------------------------------------
def mates_windows():
    """Three windows off one base.  [0]: ten reads followed by an overlapping mate under their qname (the read without its
    first 30 bases), and one read three times, the third copy behind every other read of its sample.  [1]: ten qnames shared by
    overlapping reads of samples 0 and 1, both CTRL: the second read's shared k-mers are suppressed.  [2]: ten qnames shared by
    overlapping reads of samples 0 (CTRL) and 2 (CASE): the tag of the key differs and nothing is suppressed."""
    out = []
    win = base_window("mates")
    passing = [r for r in win["reads"] if r["passf"]]
    mates = {id(r): _copy(r, seq=r["seq"][30:].copy(), qual=r["qual"][30:].copy(), start=r["start"] + 30) for r in passing[:40:4]}
    thrice = passing[50]
    reads = []
    for r in win["reads"]:
        reads.append(r)
        if id(r) in mates:
            reads.append(mates[id(r)])
        if r is thrice:
            reads.append(_copy(r))
    last = max(i for i, r in enumerate(reads) if r["passf"] and r["sample"] == thrice["sample"])
    reads.insert(last + 1, _copy(thrice))
    out.append(dict(ref=win["ref"], reads=reads))
    for other in (1, 2):
        win = base_window("mates")
        passing = [r for r in win["reads"] if r["passf"]]
        first = [r for r in passing if r["sample"] == 0]
        second = [r for r in passing if r["sample"] == other]
        shared = 0
        for x in first[::3]:
            y = next((y for y in second if abs(y["start"] - x["start"]) <= 60 and "taken" not in y), None)
            if y is not None and shared < 10:
                y["qname"], y["taken"] = x["qname"], True
                shared += 1
        assert shared == 10
        for r in win["reads"]:
            r.pop("taken", None)
        out.append(win)
    return out


# ---- the expected-error gate -------------------------------------------------------------------------------------------
def echo_pattern():
    """150 qualities: a 25-base pattern of nine Q10 and ten Q20 among Q255 (whose 10^-25.5 vanishes in the sum), 100 bases of
    Q2, and the pattern again.  9 x 0.1 + 10 x 0.01 is 1 on paper.  The k-mer on the first copy has a fresh sum just below 1.0
    and passes; for the one on the second copy the difference of two accumulators above 64 (steps of 1.4e-14: every 0.1 is
    rounded down by 0.4 of a step, every 0.01 up by 0.36) is exactly 1.0, and the gate refuses it.  The first arrangement of
    the pattern for which both hold."""
    for seed in range(400):
        rng = np.random.default_rng(9000 + seed)
        pat = np.full(25, 255, np.uint8)
        order = rng.permutation(25)
        pat[order[:9]], pat[order[9:19]] = 10, 20
        q = np.concatenate([pat, np.full(100, 2, np.uint8), pat])
        acc, prefix = 0.0, [0.0]
        for x in q:
            acc += PHRED_ERR[int(x)]
            prefix.append(acc)
        if prefix[25] - prefix[0] < 1.0 == prefix[150] - prefix[125]:
            return q
    raise AssertionError("no arrangement found")


def boundary_pattern(lo, hi, at=60):
    """150 qualities of Q2 with 25 bases of Q10 - Q13 and Q41 at `at` whose expected errors, taken as the difference of the two
    prefix sums, lie in [lo, hi): the first drawing that does.  Every other k-mer of the read holds a Q2 base beside at least
    24 bases of the pattern, 0.63 + 0.9 or more, and is refused."""
    for seed in range(4000):
        rng = np.random.default_rng(12000 + seed)
        pat = np.where(rng.random(25) < 0.55, rng.integers(10, 14, 25), 41).astype(np.uint8)
        q = np.full(150, 2, np.uint8)
        q[at:at + 25] = pat
        acc, prefix = 0.0, [0.0]
        for x in q:
            acc += PHRED_ERR[int(x)]
            prefix.append(acc)
        if lo <= prefix[at + 25] - prefix[at] < hi:
            return q
    raise AssertionError("no pattern found")


def decisive_bubble(win, p, quals, at):
    """A bubble at site p that stands or falls with ONE gate verdict.  Three CTRL reads of sample 0 carry a new base at p: one
    whole, one cut behind the k-mer that starts at p - 13, one cut in front of the k-mer that starts at p - 11 -- every k-mer
    of the bubble has the counts (2, 0, 0), total = min_node_cov, but the one that starts at p - 12, which has (1, 0, 0).  A
    fourth read of that sample, made of the reference with the new base, holds that k-mer at offset `at` under the qualities
    `quals`.  Counted there, the k-mer has (2, 0, 0) and the bubble is whole; refused, the k-mer is a singleton, goes in the first
    low-coverage pass, and the two halves are tips of 12 k-mers, which go too.  Returns the k-mer."""
    ref = bytes(win["ref"])
    alt = _other(ref[p])
    seen, three = set(), []
    for r, o in holders(win, p, K, K + 1, 0):
        if r["qname"] not in seen and len(three) < 3:
            seen.add(r["qname"])
            three.append((r, o))
    assert len(three) == 3
    for i, (r, o) in enumerate(three):
        seq = r["seq"].copy()
        seq[o] = alt
        seq = (seq, seq[:o + 12], seq[o - 11:])[i]
        r["seq"], r["qual"] = seq.copy(), np.full(len(seq), 36, np.uint8)
    start = p - 12 - at
    assert 0 <= start and start + 150 <= len(ref)
    seq = np.frombuffer(ref[start:start + 150], np.uint8).copy()
    seq[12 + at] = alt
    whole = three[0][0]
    fourth = _copy(whole, seq=seq, qual=np.asarray(quals, np.uint8).copy(), qname=_new_qname(win), rev=False, start=start, hint=start)
    idx = next(i for i, r in enumerate(win["reads"]) if r is whole)
    win["reads"].insert(idx + 1, fourth)
    return ref[p - 12:p] + bytes([alt]) + ref[p + 1:p + 13]


def gate_window():
    """Every eighth passing read gets qualities of Q41 with Q10 - Q13 bases at a density at which the 25-base sums of
    10^(-q/10) scatter around 1.0 (about 0.55: 13.7 such bases of 0.073 on average).  Three sites carry a decisive_bubble(): one
    decided by echo_pattern() (refused at exactly 1.0 only because the error is a prefix difference: the fresh sum is below 1.0), one by an instance in [0.9985, 0.9999) (counted: the bubble is in the graph), one by an instance in
    [1.0001, 1.0015) (refused: it is not).  Returns the window and the three deciding k-mers."""
    win = base_window("gate")
    rng = np.random.default_rng(4242)
    passing = [r for r in win["reads"] if r["passf"]]
    for r in passing[::8]:
        n = len(r["qual"])
        r["qual"] = np.where(rng.random(n) < 0.55, rng.integers(10, 14, n), 41).astype(np.uint8)
    sites = [p for p in clean_sites(win, K, K + 1) if p >= 140]
    assert len(sites) >= 3, sites
    kmers = [decisive_bubble(win, sites[0], echo_pattern(), 125),
             decisive_bubble(win, sites[1], boundary_pattern(0.9985, 0.9999), 60),
             decisive_bubble(win, sites[2], boundary_pattern(1.0001, 1.0015), 60)]
    return win, kmers


# ---- labels ------------------------------------------------------------------------------------------------------------
def labels_window():
    """A CASE-only bubble (every second plain CASE read at site 0 gets another base) and a bubble whose first inserter is a
    CTRL read and which CASE reads support too (every second plain read of every sample at site 1).  Returns the window and the
    two alternative 2k - 1 contexts."""
    win = base_window("labels")
    ref = bytes(win["ref"])
    sites = clean_sites(win, K, K + 1)
    assert len(sites) >= 2
    alts = []
    for p, sample in ((sites[0], 2), (sites[1], None)):
        alt = _other(ref[p])
        for r, o in holders(win, p, K, K + 1, sample)[::2]:
            r["seq"][o] = alt
        alts.append(ref[p - K + 1:p] + bytes([alt]) + ref[p + 1:p + K])
    return win, alts


# ---- singletons --------------------------------------------------------------------------------------------------------
def singletons_window():
    """One read of each of the three samples carries the same new base at site 0, one read of samples 0 and 2 at site 1: the
    k-mers over it have the counts (1, 1, 1) and (1, 0, 1), totals 3 and 2 >= min_node_cov, and are removed all the same."""
    win = base_window("singletons")
    ref = bytes(win["ref"])
    sites = clean_sites(win, K, K + 1)
    assert len(sites) >= 2
    for p, samples in ((sites[0], (0, 1, 2)), (sites[1], (0, 2))):
        for s in samples:
            r, o = holders(win, p, K, K + 1, s)[1]
            r["seq"][o] = _other(ref[p], 2)
    return win


# ---- tips and chains ---------------------------------------------------------------------------------------------------
def tips_window():
    """Read-only branches, three reads of one sample each (site, what): (0) reads cut at the site and continued with k - 1 new
    bases -- a tip of uniq_len k - 1, removed; (1) the same with k new bases -- uniq_len == k, kept, a dead end no walk
    crosses; (2) a stem of 10 new bases that forks into two ends of 10: the first round removes the ends, the second the stem;
    (3) a branch that joins the reference from outside -- 30 new bases, a run of k + 5 A, 5 new bases, then the read from the
    site on: the k-mer of A alone has an edge to itself and must stay a node of its own; no walk from the source enters the
    branch, so the cycle test does not see it.  (What this shows is that the node is built, kept and exported as it is, loop
    edges and all.  It does not make HasSelfLoop decisive: AddNodes stores a loop as two edges of the node, ++ and --, so with
    its way in and out the node has four, and the one-or-two-edges test bars every merge before the loop test is asked; a
    loop node with two edges or fewer has no other neighbour.)  Returns the window and the new sequences (kept tip, removed
    tip)."""
    win = base_window("tips")
    ref = bytes(win["ref"])
    rng = np.random.default_rng(777)
    sites = clean_sites(win, 45, 45, per_sample=6, gap=140)
    assert len(sites) >= 4, sites

    def novel(n, not_first=None, not_last=None):
        while True:
            s = bytes(synth.BASES[rng.integers(0, 4, n)])
            if s[0] != not_first and s[-1] != not_last and b"AAAA" not in s:
                return s

    def put(r, seq):
        r["seq"] = np.frombuffer(seq, np.uint8).copy()
        r["qual"] = np.full(len(seq), 36, np.uint8)

    short, kept = novel(K, ref[sites[0]]), novel(K + 1, ref[sites[1]])
    for site, tail, sample in ((sites[0], short, 0), (sites[1], kept, 0)):
        for r, o in holders(win, site, 45, 45, sample)[:3]:
            put(r, bytes(r["seq"][:o]) + tail)
    stem = novel(10, ref[sites[2]])
    end_a = novel(10)
    end_b = novel(10, end_a[0])
    for i, (r, o) in enumerate(holders(win, sites[2], 45, 45, 1)[:6]):
        put(r, bytes(r["seq"][:o]) + stem + (end_a if i % 2 else end_b))
    head = novel(30, None, ord("A")) + b"A" * (K + 5) + novel(5, ord("A"), ref[sites[3] - 1])
    for r, o in holders(win, sites[3], 45, 45, 2)[:3]:
        put(r, head + bytes(r["seq"][o:]))
    return win, (kept, short)


# ---- N bases and filtered reads ----------------------------------------------------------------------------------------
def nfilt_window():
    """A CASE-only bubble at site 0; two of its reads have an N three bases behind the new base (quality kept: the k-mers that
    hold the N are counted and stay in the graph as they are); four reads that fail the filter carry a third base at the site
    and four more the bubble's: counted, they would add a branch and raise the bubble's counts."""
    win = base_window("nfilt")
    ref = bytes(win["ref"])
    p = clean_sites(win, K, K + 1, per_sample=8)[0]
    alt, third = _other(ref[p]), _other(ref[p], 2)
    hold = holders(win, p, K, K + 1, 2)
    for r, o in hold[::2]:
        r["seq"][o] = alt
    for r, o in hold[0:4:2]:
        r["seq"][o + 3] = ord("N")
    qn = _new_qname(win)
    for i, (r, o) in enumerate(hold[1:9]):
        c = _copy(r, qname=qn + i, passf=False)
        c["seq"][o] = third if i % 2 else alt
        win["reads"].append(c)
    return win


HANDMADE = ("mates_overlap", "mates_same_role", "mates_other_role", "gate", "labels", "singletons", "tips", "nfilt")


@functools.lru_cache(maxsize=None)
def handmade():
    """dict(name -> window), the names in HANDMADE order, and what the windows' builders return beside them"""
    m = mates_windows()
    lab, alts = labels_window()
    tips, tails = tips_window()
    gate, gate_kmers = gate_window()
    wins = dict(zip(HANDMADE, (m[0], m[1], m[2], gate, lab, singletons_window(), tips, nfilt_window())))
    return wins, dict(label_alts=alts, tip_tails=tails, gate_kmers=gate_kmers)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case(params, arrs, n, nr, caps, min_compared, three_routes, handmade)"""
    def case(params, batch, min_compared, caps=ROOMY, three_routes=False, hm=False):
        arrs, n, nr = batch
        return types.SimpleNamespace(params=params, arrs=arrs, n=n, nr=nr, caps=caps, min_compared=min_compared,
                                     three_routes=three_routes, handmade=hm)
    k25 = dict(min_k=K, max_k=K)
    wins, _ = handmade()
    return dict(
        c2=case(capi.default_params(**k25), synth.make_config_batch("C2", 8, first_index=40_000), 4, three_routes=True),
        c3_ladder=case(capi.default_params(), synth.make_config_batch("C3", 6, first_index=43_000, tandem_dup=40, softclip_frac=0.03), 4),
        c5_three_samples=case(capi.default_params(num_samples=3, **k25), synth.make_config_batch("C5", 4, first_index=44_000), 4),
        c4_deep=case(capi.default_params(**k25), synth.make_config_batch("C4", 1, first_index=91_002), 1, caps=(4096, 16384, 262144)),
        handmade=case(capi.default_params(num_samples=3, **k25), synth.pack_batch([wins[name] for name in HANDMADE]), len(HANDMADE),
                      three_routes=True, hm=True))


# ---- what both test files do with a case -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built(name, w, k):
    """graph_build_ref.build_window on window w of a case, once per (case, window, k)"""
    import graph_build_ref
    c = cases()[name]
    return graph_build_ref.build_window(c.arrs, w, k, c.params)


def expected_arrays(name, w, asm):
    """The restatement's graph of window w at asm's win_k, laid out as ma_graph_out_t with the components in the order of the
    comp_* rows of `asm` (the engine's or the oracle's): matched by comp_anchor, and every row must find its component."""
    import graph_build_ref
    c = cases()[name]
    bw = built(name, w, int(asm["win_k"][w]))
    by_anchor = {e["anchor"]: e for e in bw}
    assert len(by_anchor) == len(bw)
    rows = [int(asm["comp_anchor"][w * c.params.max_comps + i]) for i in range(int(asm["win_ncomp"][w]))]
    missing = [a for a in rows if a not in by_anchor]
    assert not missing, f"{name} w{w}: no pruned component of the restatement starts at {missing}; it has {sorted(by_anchor)}"
    return graph_build_ref.to_export_arrays([by_anchor[a] for a in rows], c.params.num_samples)


UNSPECIFIED = capi.MA_W_TABLE_OVERFLOW | capi.MA_W_HAP_OVERFLOW | capi.MA_W_LEN_OVERFLOW


def comparable(asm, w):
    """a window with a result whose export is specified"""
    return int(asm["win_ncomp"][w]) > 0 and not int(asm["win_status"][w]) & UNSPECIFIED
