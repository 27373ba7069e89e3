"""The inputs of tests/test_probe_cases.py (CPU) and tests/test_gpu_probes.py: probe lists over four cases of
tests/graph_build_cases.py -- handmade, c2, c3_ladder (k above 32) and c5_three_samples -- and one new hand-made window (`gap`);
for the GPU file also `edges` (that window four times: as it is, without reads, without probes, as it is) and `retry` (the
batch whose search arena tests/test_gpu_graph_export.py forces too small).

Per window: every (variant, ALT) the oracle's MSA reports; SNV decoys at offsets 0, 1, 300 and the last base (contexts clipped
at the window's ends: 1, 2, 25 and 1 ALT-unique k-mers at k = 25); a 40-base insertion and a 30-base deletion that are nowhere
in the reads.  Planted, from the builders' own facts: the two sites of singletons_window with the base its reads carry, the two
tails of tips_window as equal-length replacements, and in `gap` a probe that adds a fake SNV between two real ones.
Everything here is data; what the rows must be is tests/probe_ref.py's business."""
import functools
import types

import numpy as np

import graph_build_cases as gc
import graph_build_ref as gb
import probe_ref as pr
from harness import OracleEngine, haplotypes_of, variants_of
from lancet2_amd import capi, synth

K = gc.K
NAMES = ("handmade", "c2", "c3_ladder", "c5_three_samples", "gap")
W_SINGLETONS, W_TIPS = gc.HANDMADE.index("singletons"), gc.HANDMADE.index("tips")
GAP_SEED, GAP_DIST = 3110, 20


def gap_window():
    """Two real SNVs GAP_DIST bases apart, carried together by every second plain read of every sample that spans both.
    Returns the window, the first site p, and the 21-base ALT that holds both SNVs AND a fake one half way between them: of its
    45 ALT-unique k-mers at k = 25 the first ten hold only the first SNV and the last ten only the second -- they are in the
    reads and the graph -- and the 25 between hold the fake base: one gap."""
    win = synth.make_window(GAP_SEED, **gc.HM_KW)
    ref = bytes(win["ref"])
    p = gc.clean_sites(win, K, K + GAP_DIST + 1)[0]
    a1, a2, fake = gc._other(ref[p]), gc._other(ref[p + GAP_DIST]), gc._other(ref[p + GAP_DIST // 2], 2)
    for r, o in gc.holders(win, p, K, K + GAP_DIST + 1)[::2]:
        r["seq"][o], r["seq"][o + GAP_DIST] = a1, a2
    mid = p + GAP_DIST // 2
    alt = bytes([a1]) + ref[p + 1:mid] + bytes([fake]) + ref[mid + 1:p + GAP_DIST] + bytes([a2])
    return win, p, alt


@functools.lru_cache(maxsize=None)
def case(name):
    """Case(params, arrs, n, nr) -- graph_build_cases' own, or the one window of `gap`"""
    if name in ("gap", "edges"):
        win = gap_window()[0]
        wins = [win] if name == "gap" else [win, dict(ref=win["ref"], reads=[]), win, win]
        arrs, n, nr = synth.pack_batch(wins)
        return types.SimpleNamespace(params=capi.default_params(num_samples=3, min_k=K, max_k=K), arrs=arrs, n=n, nr=nr)
    if name == "retry":  # the batch of tests/test_gpu_graph_export.py's capacity-retry test
        arrs, n, nr = synth.make_config_batch("C2", 12, first_index=77_000, snv_rate=1e-2, indel_rate=2e-3)
        return types.SimpleNamespace(params=capi.default_params(min_k=K, max_k=K), arrs=arrs, n=n, nr=nr)
    return gc.cases()[name]


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """(asm, var) of the oracle on the case"""
    c = case(name)
    orc = OracleEngine(c.params)
    asm = orc.assemble(c.arrs, c.n, c.nr)
    var = orc.msa(c.arrs, c.n, c.nr, {k: v.copy() for k, v in asm.items()})
    return asm, var


def window_ref(c, w):
    return bytes(c.arrs["ref_bases"][int(c.arrs["ref_off"][w]):int(c.arrs["ref_off"][w + 1])])


def _snv(ref, o, step=1):
    return (o, 1, bytes([gc._other(ref[o], step)]) if ref[o] in b"ACGT" else b"A")


@functools.lru_cache(maxsize=None)
def probes(name):
    """per window: [(pos, ref_len, alt, tag)], tag = "oracle", "decoy", "absent" or a planted probe's name"""
    c = case(name)
    _, var = oracle_run(name)
    out = []
    for w in range(c.n):
        ref = window_ref(c, w)
        L = len(ref)
        lst, seen = [], set()
        for pos, refa, alts in variants_of(c.params, var, w):
            for alt in alts:
                key = (pos, len(refa), alt)
                if key not in seen and len(alt) <= capi.PROBE_MAX_ALLELE and len(refa) <= capi.PROBE_MAX_ALLELE:
                    seen.add(key)
                    lst.append(key + ("oracle",))
        for o in (0, 1, 300, L - 1):
            lst.append(_snv(ref, o) + ("decoy",))
        rng = np.random.default_rng(5000 + 97 * sum(name.encode()) + w)
        lst.append((500, 1, ref[500:501] + bytes(synth.BASES[rng.integers(0, 4, 40)]), "absent"))
        lst.append((600, 31, ref[600:601], "absent"))
        if name == "handmade" and w == W_SINGLETONS:
            sites = gc.clean_sites(gc.base_window("singletons"), K, K + 1)
            lst += [_snv(ref, sites[0], 2) + ("singleton0",), _snv(ref, sites[1], 2) + ("singleton1",)]
        if name == "handmade" and w == W_TIPS:
            sites = gc.clean_sites(gc.base_window("tips"), 45, 45, per_sample=6, gap=140)
            kept, short = gc.handmade()[1]["tip_tails"]
            lst += [(sites[0], len(short), short, "tip_short"), (sites[1], len(kept), kept, "tip_kept")]
        if name in ("gap", "edges"):
            _, p, alt = gap_window()
            lst.append((p, GAP_DIST + 1, alt, "gap"))
        if name == "edges" and w == 2:
            lst = []
        assert len(lst) <= capi.PROBE_MAX_PER_WINDOW
        out.append(lst)
    return out


def packed(name, per_window=None):
    """capi.pack_probes of the case's probes"""
    return capi.pack_probes([[p[:3] for p in lst] for lst in (per_window if per_window is not None else probes(name))])


@functools.lru_cache(maxsize=None)
def _built(name, w, k):
    c = case(name)
    return gc.built(name, w, k) if name in gc.cases() else gb.build_window(c.arrs, w, k, c.params)


@functools.lru_cache(maxsize=None)
def _lowcov1(name, w, k):
    c = case(name)
    ref, reads = gb.window_inputs(c.arrs, w)
    return pr.lowcov1_kmers(ref, reads, k, c.params)


def expected_rows(name, asm, per_window=None, case_obj=None):
    """per window, probe_ref.window_rows at asm's win_k with the components and haplotypes of asm's rows (the engine's or the
    oracle's).  pb_final is None where the window's graph is unspecified (graph_build_cases.comparable), pb_lowcov1 where the
    window is left MA_W_TABLE_OVERFLOW.  case_obj: a batch that is none of the named cases (then per_window is required)."""
    c = case_obj or case(name)
    built = _built if case_obj is None else (lambda _, w, k: gb.build_window(c.arrs, w, k, c.params))
    lowcov1 = _lowcov1 if case_obj is None else (lambda _, w, k: pr.lowcov1_kmers(*gb.window_inputs(c.arrs, w), k, c.params))
    lists = per_window if per_window is not None else probes(name)
    out = []
    for w in range(c.n):
        k = int(asm["win_k"][w])
        ref, reads = gb.window_inputs(c.arrs, w)
        ncomp = int(asm["win_ncomp"][w])
        comp_nodes = []
        if ncomp > 0:
            comp_nodes = None
            if gc.comparable(asm, w):
                by_anchor = {e["anchor"]: e for e in built(name, w, k)}
                rows = [int(asm["comp_anchor"][w * c.params.max_comps + i]) for i in range(ncomp)]
                assert all(a in by_anchor for a in rows), (name, w, rows, sorted(by_anchor))
                comp_nodes = [[nd["seq"] for nd in by_anchor[a]["nodes"]] for a in rows]
        lists_w = [p[:3] for p in lists[w]]
        low = lowcov1(name, w, k) if k and lists_w else set()
        rows = pr.window_rows(ref, reads, k, lists_w, c.params.max_comps, low, comp_nodes, haplotypes_of(c.params, asm, w))
        if int(asm["win_status"][w]) & capi.MA_W_TABLE_OVERFLOW:
            for r in rows:
                r["pb_lowcov1"] = r["pb_final"] = None
        out.append(rows)
    return out


def engine_rows(name, po, per_window=None):
    """the engine's arrays, window by window, as expected_rows lays them out"""
    c = case(name)
    lists = per_window if per_window is not None else probes(name)
    out, p = [], 0
    for w in range(c.n):
        out.append([pr.engine_row(po, p + i, c.params.max_comps) for i in range(len(lists[w]))])
        p += len(lists[w])
    return out


def compare_case(name, got, want):
    bad = []
    for w, (g, x) in enumerate(zip(got, want)):
        bad += pr.compare(g, x, f"{name} w{w}")
    return bad
