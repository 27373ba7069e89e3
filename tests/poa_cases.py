"""Hand-made components for the POA stage (Engine.msa against OracleEngine.msa) at the engine's capacity edges: what
tests/scoring_cases.py is for the genotyper.  Inputs only -- nothing here looks at either implementation.

poa.hip keeps structure the oracle's POA does not have: kPE = 4 out-edges, in-edges and aligned nodes per graph node, a
node capacity `pn` sized from the longest haplotype of the BATCH (so it depends on batch mates), one LDS block per window
(which bounds the haplotype length), a run-length chain over four wavefronts in the bubble walk and five column-width
classes of the full fill.  Every window below is a REF haplotype from a seeded rand_dna plus ALT haplotypes given as edit
lists, placed so that one of those structures is at its exact fit or one over:

  edit = ("snv", p, base) | ("del", p, L)  (deletes ref[p:p+L]) | ("ins", p, seq)  (seq goes in front of ref[p])

Where a case relies on WHERE an indel sits, the REF is re-drawn until the place is unique (a deletion ref[p:p+L] cannot
shift: ref[p-1] != ref[p+L-1] and ref[p] != ref[p+L]; an insertion neither: seq[-1] != ref[p-1], seq[0] != ref[p]), so the
graph degrees are what the table says and not what a tie rule made of them.  shape() computes them from the edit lists.

may_flag: the engine may answer the window with a capacity flag instead of variants (a capped window is
compared by status only).  Only the "over" cases (a kPE width or the node capacity exceeded by construction), the headroom
cases whose fit depends on pn, and the long cases (a haplotype beyond what one LDS block can hold) carry it."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from harness import OracleEngine, handmade_poa_case
from lancet2_amd import capi, synth
from pin_cases import rand_dna

BASES = b"ACGT"
ANCHOR = 17

# A LAB32 kernel keeps 66 bytes of LDS per graph node (50 graph + 12 row descriptors + 4 path) and 4 per haplotype base,
# and a graph has at least as many nodes as its longest haplotype has bases: 70 bytes per base of a 160 KB block, state
# and slow-row table not counted -- no haplotype beyond 160 * 1024 / 70 = 2340 bases can take the LAB32 kernels at all.
# (The common kernels: 58 + 4 bytes, 2642.)  Windows longer than that are long cases on that route.
LAB32_LEN_CEILING = 160 * 1024 // 70
COMMON_LEN_CEILING = 160 * 1024 // 62


def other_base(b, k=1):
    return BASES[(BASES.index(bytes([b])) + k) % 4]


def apply_edits(ref, edits):
    b = bytearray(ref)
    for e in sorted(edits, key=lambda e: e[1], reverse=True):
        if e[0] == "snv":
            b[e[1]] = e[2]
        elif e[0] == "del":
            del b[e[1]:e[1] + e[2]]
        else:
            b[e[1]:e[1]] = e[2]
    return bytes(b)


def unique_place(ref, e):
    """the edit cannot be moved along the REF without changing the haplotype"""
    n = len(ref)
    if e[0] == "del":
        p, L = e[1], e[2]
        return (p == 0 or ref[p - 1] != ref[p + L - 1]) and (p + L >= n or ref[p] != ref[p + L])
    if e[0] == "ins":
        p, s = e[1], e[2]
        return (p == 0 or s[-1] != ref[p - 1]) and (p >= n or s[0] != ref[p])
    return True


def shape(ref, alts):
    """-> (largest out-degree, largest in-degree, largest aligned ring) of the graph that the edit lists describe: REF chain
    plus every ALT haplotype's path, a substituted base aligned to the REF node it replaces"""
    edges, ring = set(), {}
    for p in range(len(ref) - 1):
        edges.add((p, p + 1))
    for edits in alts:
        path, at = [], 0
        for e in sorted(edits, key=lambda e: e[1]):
            path.extend(range(at, e[1]))
            at = e[1]
            if e[0] == "snv":
                path.append(("s", e[1], e[2]))
                ring.setdefault(e[1], {ref[e[1]]}).add(e[2])
                at += 1
            elif e[0] == "del":
                at += e[2]
            else:
                path.extend(("i", e[1], e[2], k) for k in range(len(e[2])))
        path.extend(range(at, len(ref)))
        edges.update(zip(path, path[1:]))
    out, inn = {}, {}
    for a, b in edges:
        out[a] = out.get(a, 0) + 1
        inn[b] = inn.get(b, 0) + 1
    return max(out.values()), max(inn.values()), max([len(s) for s in ring.values()] + [1])


def new_nodes(alts):
    """graph nodes beyond the REF chain (no two ALT haplotypes of a case share an edit, except where they share all)"""
    seen, n = set(), 0
    for edits in alts:
        for e in edits:
            if e in seen:
                continue
            seen.add(e)
            n += 1 if e[0] == "snv" else (len(e[2]) if e[0] == "ins" else 0)
    return n


@dataclass
class Comp:
    ref: bytes
    alts: list  # one edit list per ALT haplotype
    anchor: int = ANCHOR

    def haps(self):
        return [self.ref] + [apply_edits(self.ref, e) for e in self.alts]


@dataclass
class Window:
    name: str
    comps: list
    may_flag: bool = False
    kind: str = ""          # "over" / "headroom" / "long" for the may_flag windows; "long_lab32": long on the forced LAB32 route only
    claims: tuple = None    # (out-degree, in-degree, ring) the table claims for comps[0]
    n_alleles: int = None   # degree / ring cases: ALT alleles of the one site
    truth: list = None      # biallelic cases: [(var_pos, ref allele, (alt alleles...), {haplotype: allele index})] of comps[0]

    def max_len(self):
        return max(len(h) for c in self.comps for h in c.haps())

    def wide(self):
        return max(len(c.haps()) for c in self.comps) > 16


@dataclass
class Group:
    name: str
    params: object
    windows: list
    routes: bool            # also run under the POA's route switches
    by_name: dict = field(default_factory=dict)

    def __post_init__(self):
        self.by_name = {w.name: i for i, w in enumerate(self.windows)}
        assert len(self.by_name) == len(self.windows)


def _draw_ref(seed, n, edits_of, no_repeat=None, tries=4000):
    """a seeded REF of n bases on which every edit that edits_of(ref) plants sits at a unique place; no_repeat = (lo, hi): no
    two equal neighbours in ref[lo:hi]"""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        ref = rand_dna(rng, n)
        if no_repeat and any(ref[i] == ref[i + 1] for i in range(no_repeat[0], no_repeat[1] - 1)):
            continue
        alts = edits_of(ref, rng)
        if all(unique_place(ref, e) for edits in alts for e in edits):
            return ref, alts
    raise AssertionError("no REF with unique edit places")


def _snv(ref, p, k=1):
    return ("snv", p, other_base(ref[p], k))


def _snv_truth(ref, p, base, hap, anchor=ANCHOR):
    return (anchor + p, ref[p:p + 1], (bytes([base]),), {hap: 1})


def _del_truth(ref, p, L, hap, anchor=ANCHOR):
    return (anchor + p - 1, ref[p - 1:p + L], (ref[p - 1:p],), {hap: 1})


def _ins_truth(ref, p, seq, hap, anchor=ANCHOR):
    return (anchor + p - 1, ref[p - 1:p], (ref[p - 1:p] + seq,), {hap: 1})


def _plain(name, seed, n=700):
    """an ordinary window: two ALT haplotypes, an SNV and a 4-base deletion"""
    ref, alts = _draw_ref(seed, n, lambda r, g: [[_snv(r, 200)], [("del", 400, 4), _snv(r, 90, 2)]])
    return Window(name, [Comp(ref, alts)])


# ---- run boundaries of the bubble walk ----
RUN_DISTANCES = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300)


def _run_windows():
    ws = []
    for i, d in enumerate(RUN_DISTANCES):
        n, p = 600 + 27 * i, 100 + i  # (a converged stretch of p nodes in front, d - 1 between the two sites, the rest behind)
        ref, alts = _draw_ref(5000 + i, n, lambda r, g, p=p, d=d: [[_snv(r, p), _snv(r, p + d, 2)]])
        (_, _, b1), (_, _, b2) = alts[0]
        if d == 1:  # adjacent substitutions never converge in between: one bubble, one 2-base MNP
            truth = [(ANCHOR + p, ref[p:p + 2], (bytes([b1, b2]),), {1: 1})]
        else:
            truth = [_snv_truth(ref, p, b1, 1), _snv_truth(ref, p + d, b2, 1)]
        ws.append(Window(f"snv_pair_d{d}", [Comp(ref, alts)], truth=truth))
    n = 640
    for name, off in (("snv_first", 0), ("snv_second", 1), ("snv_last_but_one", n - 2), ("snv_last", n - 1)):
        ref, alts = _draw_ref(5100 + off, n, lambda r, g, off=off: [[_snv(r, off)]])
        ws.append(Window(name, [Comp(ref, alts)], truth=[_snv_truth(ref, off, alts[0][0][2], 1)]))
    # indels that touch an end: the last-base ones have a base in front (VCF's anchor base); the first-base ones have none
    ref, alts = _draw_ref(5201, n, lambda r, g: [[("del", n - 3, 3)]])
    ws.append(Window("del3_ends_on_last", [Comp(ref, alts)], truth=[_del_truth(ref, n - 3, 3, 1)]))
    ref, alts = _draw_ref(5202, n, lambda r, g: [[("ins", n, rand_dna(g, 3))]])
    ws.append(Window("ins3_behind_last", [Comp(ref, alts)], truth=[_ins_truth(ref, n, alts[0][0][2], 1)]))
    ref, alts = _draw_ref(5203, n, lambda r, g: [[("del", 0, 3)]])
    # no base in front: the bubble opens without an anchor base, the alleles are ref[0:3] against the empty string
    ws.append(Window("del3_starts_on_first", [Comp(ref, alts)], truth=[(ANCHOR, ref[0:3], (b"",), {1: 1})]))
    ref, alts = _draw_ref(5204, n, lambda r, g: [[("ins", 0, rand_dna(g, 3))]])
    ws.append(Window("ins3_in_front_of_first", [Comp(ref, alts)], truth=[(ANCHOR, b"", (alts[0][0][2],), {1: 1})]))
    return ws


# ---- kPE: out-degree, in-degree, aligned ring ----
# Deletions of 1, 2, ... n bases that start (end) at one base.  Once the graph holds the edge of the deletion that is one base
# shorter, the next haplotype's alignment takes that edge for nothing and pays for ONE skipped node, which could slide along
# a homopolymer: no two equal neighbours around the site, so that node is ref[p+i] (ref[p-1-i]) and the edges are the table's.
def _out_degree(n_alts, seed, p=300):
    ref, alts = _draw_ref(seed, 800, lambda r, g: [[("del", p, 1 + i)] for i in range(n_alts)], no_repeat=(p - 2, p + n_alts + 3))
    over = n_alts + 1 > 4
    return Window(f"out_degree_{n_alts + 1}", [Comp(ref, alts)], may_flag=over, kind="over" if over else "",
                  claims=(n_alts + 1, 2, 1), n_alleles=n_alts)


def _in_degree(n_alts, seed, p=300):
    ref, alts = _draw_ref(seed, 800, lambda r, g: [[("del", p - 1 - i, 1 + i)] for i in range(n_alts)], no_repeat=(p - n_alts - 3, p + 2))
    over = n_alts + 1 > 4
    return Window(f"in_degree_{n_alts + 1}", [Comp(ref, alts)], may_flag=over, kind="over" if over else "",
                  claims=(2, n_alts + 1, 1), n_alleles=n_alts)


def _ring(extra, seed, p=300):
    """one site that carries the other three of A, C, G, T, then every byte of `extra`.  A fifth base at the site alone would
    also be a fifth edge out of ref[p-1] and into ref[p+1] (the out-degree case again, not the ring's): the haplotypes of
    `extra` substitute both neighbours as well, so their ring node hangs between nodes of their own and the ring is the only
    width in question -- every degree stays 4.  The neighbours get letters that occur nowhere else (R, Y, K, M): nothing of
    the three bases matches any node, the diagonal (-18) beats every path with gaps (-20 at best), no tie rule is asked"""
    flanks = (b"RY", b"KM")
    ref, alts = _draw_ref(seed, 800, lambda r, g: [[_snv(r, p, k)] for k in (1, 2, 3)] +
                          [[("snv", p - 1, flanks[j][0]), ("snv", p, x), ("snv", p + 1, flanks[j][1])] for j, x in enumerate(extra)])
    size = 4 + len(extra)
    return Window(f"ring_{size}", [Comp(ref, alts)], may_flag=size > 5, kind="over" if size > 5 else "",
                  claims=(4, 4, size), n_alleles=size - 1)


# ---- node headroom ----
def _insertions(name, n_alts, seed, n=1000, **kw):
    def edits(r, g):
        return [[("ins", 100 + 100 * i, rand_dna(g, 60))] for i in range(n_alts)]
    ref, alts = _draw_ref(seed, n, edits)
    truth = [_ins_truth(ref, e[0][1], e[0][2], 1 + h) for h, e in enumerate(alts)]
    return Window(name, [Comp(ref, alts)], truth=truth, **kw)


def _snv_spread(name, n_snvs, seed, n, n_alts=6, **kw):
    """n_snvs substitutions at distinct sites, dealt out to n_alts haplotypes in turn, at least 7 bases apart"""
    step = (n - 100) // n_snvs
    assert step >= 7
    sites = [50 + step * j for j in range(n_snvs)]
    ref, alts = _draw_ref(seed, n, lambda r, g: [[_snv(r, s, 1 + j % 3) for j, s in enumerate(sites) if j % n_alts == h] for h in range(n_alts)])
    truth = sorted(_snv_truth(ref, e[1], e[2], 1 + h) for h, edits in enumerate(alts) for e in edits)
    return Window(name, [Comp(ref, alts)], truth=truth, **kw)


# ---- length classes ----
LENGTHS = (1024, 1025, 1536, 1537, 2048, 2049, 2400, 3072, 3073, 4096)
LONG_LENGTHS = (3072, 3073, 4096)
# The longest haplotype the stage takes today, common kernels / LAB32 kernels (launch_msa prints both under MA_VERBOSE; DESIGN
# section 7), and one more: the largest LDS block the stage ever asks for, and the first window it leaves out.
LEN_EDGE, LEN_EDGE_LAB32 = 2551, 2255


def _length_window(n, seed, kind=None, may_flag=None):
    mid = n // 2
    ref, alts = _draw_ref(seed, n, lambda r, g: [[_snv(r, 5), _snv(r, n - 1, 2)], [("del", mid, 30)], [_snv(r, n - 2, 3)]])
    a5, alast, apen = alts[0][0][2], alts[0][1][2], alts[2][0][2]
    # the substitutions at L-2 (haplotype 3) and L-1 (haplotype 1) are neighbours: the walk does not converge between them,
    # so they form ONE site ref[L-2:L] with the two ALT alleles in byte order
    tail = sorted([(ref[n - 2:n - 1] + bytes([alast]), 1), (bytes([apen]) + ref[n - 1:n], 3)])
    truth = [_snv_truth(ref, 5, a5, 1), _del_truth(ref, mid, 30, 2),
             (ANCHOR + n - 2, ref[n - 2:n], tuple(a for a, _ in tail), {h: 1 + k for k, (_, h) in enumerate(tail)})]
    if kind is None:
        kind = "long" if n in LONG_LENGTHS else ""
    return Window(f"length_{n}", [Comp(ref, alts)], may_flag=bool(kind) if may_flag is None else may_flag, kind=kind, truth=truth)


# ---- rows of the banded fill that are not straight-line ----
# poa.hip's band_flags marks a row RI_LEAN -- poa_fill_lean's straight-line body -- when it has one predecessor, the previous
# rank, no later row reads it back, it is not a sink, and its window sits where the previous row's sits or one lane to the
# right (or both start at column 1).  Every other row takes the any-shape body (row_gen).  One window per way out, on
# haplotypes of 400 bases and more (shorter ones are not banded), none of them may_flag:
#   band_store_bubbles   rows with two predecessors, the far one read back from the row store (RI_STORE): a 5-base deletion
#                        and a 6-base insertion open two bubbles; the second and the third haplotype cross both with
#                        substitutions within three bases of each branch point
#   band_col0_insertion  rows that are not FAST while the window starts at column 1: two haplotypes with an insertion within
#                        their first four bases (the second one is filled against the first one's inserted nodes)
#   band_window_jump     a window that moves by more than a lane between two ranks.  A 40-base deletion already in the graph
#                        is crossed by a later haplotype; the deletion alone leaves the backbone coordinate rising by one per
#                        rank (its far end is one more two-predecessor row), so the window also holds a 40-base insertion:
#                        its nodes count 40 coordinates on and the REF node behind them steps back by as many, 20 lanes of
#                        the 128-column tier
#   band_early_sink      a sink that is not the last rank: a haplotype that ends 30 bases early.  Ending early alone adds no
#                        sink (its last node keeps the REF's edge out), so its last base is a substitution: that node has no
#                        edge out and 30 ranks or more behind it
#   band_to_full_fill    the 128-column tier fails, the 256-column tier fails too, the alignment ends in the full fill: a
#                        150-base deletion with a 60-base insertion 10 bases behind it walks 150 columns off the backbone;
#                        a second 60-base insertion keeps the haplotype within 48 bases of the REF's length, so that it
#                        starts at the first tier
def _band_shape_windows():
    n, ws = 800, []
    ref, alts = _draw_ref(6601, n, lambda r, g: [
        [("del", 200, 5), ("ins", 500, rand_dna(g, 6)), _snv(r, 650)],
        [_snv(r, 198), _snv(r, 206), _snv(r, 499), _snv(r, 501)],
        [_snv(r, 197, 2), _snv(r, 207, 2), _snv(r, 498, 2), _snv(r, 502, 2)]], no_repeat=(190, 215))
    ws.append(Window("band_store_bubbles", [Comp(ref, alts)]))
    ref, alts = _draw_ref(6602, n, lambda r, g: [
        [("ins", 2, rand_dna(g, 5)), _snv(r, 300), _snv(r, 600)],
        [("ins", 3, rand_dna(g, 4)), _snv(r, 350), _snv(r, 620, 2)]], no_repeat=(0, 12))
    ws.append(Window("band_col0_insertion", [Comp(ref, alts)]))
    ref, alts = _draw_ref(6603, n, lambda r, g: [
        [_snv(r, 100), ("del", 300, 40)],
        [("ins", 500, rand_dna(g, 40)), _snv(r, 650)],
        [_snv(r, 150, 2), _snv(r, 520, 2), _snv(r, 700, 2)]])
    (s100, _), (ins, s650), (s150, s520, s700) = alts
    ws.append(Window("band_window_jump", [Comp(ref, alts)], truth=[
        _snv_truth(ref, 100, s100[2], 1), _snv_truth(ref, 150, s150[2], 3), _del_truth(ref, 300, 40, 1), _ins_truth(ref, 500, ins[2], 2),
        _snv_truth(ref, 520, s520[2], 3), _snv_truth(ref, 650, s650[2], 2), _snv_truth(ref, 700, s700[2], 3)]))
    ref, alts = _draw_ref(6604, n, lambda r, g: [
        [_snv(r, 200), _snv(r, n - 31), ("del", n - 30, 30)],
        [_snv(r, 400), _snv(r, 500, 2), _snv(r, n - 20, 2)]])
    ws.append(Window("band_early_sink", [Comp(ref, alts)]))
    ref, alts = _draw_ref(6605, n, lambda r, g: [
        [("del", 300, 150), ("ins", 460, rand_dna(g, 60)), ("ins", 700, rand_dna(g, 60))],
        [_snv(r, 100), _snv(r, 250, 2), _snv(r, 750, 2)]])
    (_, i460, i700), (s100, s250, s750) = alts
    ws.append(Window("band_to_full_fill", [Comp(ref, alts)], truth=[
        _snv_truth(ref, 100, s100[2], 2), _snv_truth(ref, 250, s250[2], 2), _del_truth(ref, 300, 150, 1), _ins_truth(ref, 460, i460[2], 1),
        _ins_truth(ref, 700, i700[2], 1), _snv_truth(ref, 750, s750[2], 2)]))
    return ws


def _interleave(ordinary, special):
    """every special window between two ordinary ones"""
    out, o = [], list(ordinary)
    for s in special:
        out += [o.pop(0), s]
    out += o
    assert len(o) >= 1 and all(not out[i].may_flag or (not out[i - 1].may_flag and not out[i + 1].may_flag)
                               for i in range(1, len(out) - 1)) and not out[0].may_flag and not out[-1].may_flag
    return out


@lru_cache(maxsize=None)
def groups():
    gs = []
    small = dict(min_k=25, max_k=25, max_haps=16, max_vars=128, max_alts=8, max_allele_bytes=4096)
    gs.append(Group("run", capi.default_params(**small), _run_windows(), routes=True))
    gs.append(Group("degree", capi.default_params(**small), _interleave(
        [_out_degree(2, 6002), _out_degree(3, 6003), _in_degree(2, 6012), _in_degree(3, 6013), _plain("degree_plain", 6020)],
        [_out_degree(4, 6004), _out_degree(5, 6005), _in_degree(4, 6014), _in_degree(5, 6015)]), routes=True))
    gs.append(Group("ring", capi.default_params(**small), [_ring(b"", 6100), _ring(b"Na", 6102), _ring(b"N", 6101)], routes=True))
    gs.append(Group("band_shapes", capi.default_params(**small), _interleave(
        [_plain(f"band_plain_{i}", 6610 + i) for i in range(6)], _band_shape_windows()), routes=True))
    # node headroom: the batch's longest haplotype is 1060 bases, pn <= 1060 + 256 + 7
    gs.append(Group("headroom_1k", capi.default_params(**small), _interleave(
        [_insertions("ins_2x60", 2, 6200), _snv_spread("snv_40_on_1000", 40, 6210, 1000), _plain("headroom_plain", 6220, 900)],
        [_insertions("ins_8x60", 8, 6202, may_flag=True, kind="over")]) +
        [_insertions("ins_4x60", 4, 6201, may_flag=True, kind="headroom"), _plain("headroom_plain2", 6221, 950)], routes=True))
    # ... and next to a 2400-base component: pn follows the batch's longest haplotype, the same 8 insertions may fit
    long_p = dict(small, max_hap_len=4096)
    gs.append(Group("headroom_2400", capi.default_params(**long_p), _interleave(
        [_snv_spread("snv_20_on_2400", 20, 6300, 2400), _plain("mates_plain", 6320, 900), _snv_spread("snv_20_on_2400_b", 20, 6301, 2400)],
        [_insertions("ins_8x60_beside_2400", 8, 6202, may_flag=True, kind="headroom"),
         _snv_spread("snv_80_on_2400", 80, 6310, 2400, may_flag=True, kind="headroom")]), routes=True))
    lw = {n: _length_window(n, 6400 + i) for i, n in enumerate(LENGTHS)}
    gs.append(Group("length", capi.default_params(**long_p), _interleave(
        [lw[n] for n in LENGTHS if n not in LONG_LENGTHS], [lw[n] for n in LONG_LENGTHS]), routes=False))
    # the longest haplotype that fits and one more, for either kind of kernel (the LAB32 pair are ordinary windows elsewhere)
    gs.append(Group("length_edge", capi.default_params(**long_p), [
        _plain("edge_plain_a", 6450), _length_window(LEN_EDGE, 6451, "long"), _plain("edge_plain_b", 6452),
        _length_window(LEN_EDGE + 1, 6453, "long"), _plain("edge_plain_c", 6454),
        _length_window(LEN_EDGE_LAB32, 6455, "long_lab32", False), _plain("edge_plain_d", 6456),
        _length_window(LEN_EDGE_LAB32 + 1, 6457, "long_lab32", False), _plain("edge_plain_e", 6458)], routes=False))
    # A window that takes the LAB32 kernels for its SECOND component (17 haplotypes) while its first, narrow one holds the
    # longest haplotype of the batch, between the two edges: too long for the kernels the window takes, so it is left out
    # whole, and the passes -- sized from the other windows -- must not run any of it.
    ref17, alts17 = _draw_ref(6470, 700, lambda r, g: [[_snv(r, 40 + 37 * i, 1 + i % 3)] for i in range(16)])
    narrow = _snv_spread("unused", 6, 6471, 2400, n_alts=2).comps[0]
    gs.append(Group("wide_long", capi.default_params(**dict(long_p, max_haps=32)), [
        _plain("wide_long_plain_a", 6472), Window("narrow_2400_then_17_haplotypes", [narrow, Comp(ref17, alts17, ANCHOR + 3000)],
                                                  may_flag=True, kind="long"),
        _plain("wide_long_plain_b", 6473)], routes=False))
    # several components in a window: what a capped component does to the ones before and behind it
    fit_a, fit_b, fit_c = _out_degree(2, 6500).comps[0], _in_degree(3, 6501).comps[0], _ring(b"N", 6502).comps[0]
    over = _out_degree(5, 6503).comps[0]
    fit_b.anchor, fit_c.anchor, over.anchor = ANCHOR + 1000, ANCHOR + 2000, ANCHOR + 1000
    gs.append(Group("multi", capi.default_params(**small), [
        _plain("multi_plain", 6510), Window("three_fitting_components", [fit_a, fit_b, fit_c]),
        Window("over_between_two_fitting", [fit_a, over, fit_c], may_flag=True, kind="over"), _plain("multi_plain2", 6511)], routes=False))
    return {g.name: g for g in gs}


ROUTE_GROUPS = tuple(n for n in ("run", "degree", "ring", "band_shapes", "headroom_1k", "headroom_2400"))
# the switches the suite already uses to force the POA's other routes (test_gpu_parity.py, test_gpu_wide_components.py)
ROUTES = {"default": {}, "host_rounds": {"MA_POA_SCHED": "0"}, "full_fill": {"MA_POA_BAND": "0"}, "no_direct": {"MA_POA_NO_DIRECT": "1"},
          "lab32": {"MA_POA_FORCE_LAB32": "1"}, "raw_cap": {"MA_POA_RAW_CAP": "4"}}


def may_flag_on(route, w):
    """(may_flag, the flag): the table's may_flag, plus -- on the forced LAB32 route only -- the windows no LAB32 kernel can
    hold (LAB32_LEN_CEILING), which are long cases there"""
    if w.kind == "long" or (route == "lab32" and (w.kind == "long_lab32" or w.max_len() > LAB32_LEN_CEILING)):  # (long: flagged, never run)
        return True, capi.MA_W_LEN_OVERFLOW
    return w.may_flag, capi.MA_W_VAR_OVERFLOW


def build(group):
    """-> (arrs, n, nr, asm) of a group: the hand-made assembly buffers and a batch of as many windows (the POA stage reads
    only the batch's window count)"""
    g = groups()[group]
    n = len(g.windows)
    asm = handmade_poa_case(g.params, [[(c.haps(), c.anchor) for c in w.comps] for w in g.windows])
    arrs, n2, nr = synth.make_config_batch("C1", n, first_index=77)
    assert n2 == n
    return arrs, n, nr, asm


@lru_cache(maxsize=None)
def oracle_msa(group):
    """the oracle's variants of a group and the window status it leaves, computed once; callers do not write to either"""
    g = groups()[group]
    arrs, n, nr, asm = build(group)
    var = OracleEngine(g.params).msa(arrs, n, nr, asm)
    for a in list(var.values()) + [asm["win_status"]]:
        a.setflags(write=False)
    return var, asm["win_status"]
