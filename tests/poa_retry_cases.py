"""Hand-made components for the POA stage's retry passes (ma_set_poa_retry; Engine.set_poa_retry): the case table of
tests/test_gpu_poa_retry.py, built with the builders of tests/poa_cases.py.  Inputs only.

With the setting on, a window whose POA graph ran out of per-node slots (four in / out edges, a node and four aligned ones)
or of nodes (a capacity sized from the batch's longest haplotype) is re-run by a second pass: eight slots per node, or four
and as many nodes as one LDS block holds.  tests/poa_cases.py has what the first pass flags; here is what the SECOND pass
holds at its exact fit and flags one over:

  degree8  eight edges out of / into one node (exact fit), nine (one over; eight ALT alleles are max_alts exactly)
  ring9    a site with nine letters (a node and eight aligned ones: exact fit), ten (one over; max_alts = 12)
  nodes    12 x 60 inserted bases on 1000 (720 new nodes: more than the first pass has, fewer than the block holds),
           15 x 120 (1800 new nodes beside 1120-base haplotypes: more than the block holds)
  both     a window whose first component is over for its width and whose second for its nodes; a window of three components
           with the capped one in the middle

Every special window sits between ordinary ones.  kind: "fit" -- flagged by the first pass, called by the retry; "over" --
flagged by both (may_flag, compared by status only)."""
from functools import lru_cache

from harness import OracleEngine, handmade_poa_case
from lancet2_amd import capi, synth
from pin_cases import rand_dna
from poa_cases import ANCHOR, Comp, Group, Window, _draw_ref, _in_degree, _insertions, _interleave, _out_degree, _plain, _ring, _snv

# LDS bytes of one window (poa.hip: poa_lds_bytes), restated from DESIGN section 7 so that the table can say which side of
# the retry's capacities a case lies on: state block 1776, 16 of padding; per node 10 + pe * 8 of graph (16-bit labels), 12 of
# row descriptors, 4 of path; 2 * pe * 256 of slow-row table; 4 per haplotype base; the block: 160 KB less 256
LDS_BLOCK = 160 * 1024 - 256


def node_capacity(max_len, pe):
    """the most nodes (a multiple of 8) a retry pass has for haplotypes of max_len bases with pe slots per node"""
    fixed = 1776 + 16 + 24 + 2 * pe * 256 + 4 * (max_len + 2)
    return (LDS_BLOCK - fixed) // (10 + pe * 8 + 16) // 8 * 8


def _retag(w, fit):
    """the poa_cases builders tag by the first pass's widths; here a case is "fit" (the retry holds it) or "over" (it does not)"""
    w.may_flag, w.kind = (not fit), ("fit" if fit else "over")
    return w


def _ring_n(extra, seed, p=300):
    """poa_cases._ring for any number of extra letters: one site that carries the other three of A, C, G, T, then every byte
    of `extra`, each on a haplotype that substitutes both neighbours as well, with a pair of letters that occurs nowhere else
    (see _ring: the ring node then hangs between nodes of the haplotype's own, nothing of the three bases matches any node,
    the diagonal wins without a tie).  Every such haplotype adds an edge out of ref[p-2] and into ref[p+2] and a node to the
    rings of the two neighbours: 1 + len(extra) each, below the site's own ring of 4 + len(extra)"""
    flanks = (b"RY", b"KM", b"BD", b"HV", b"SW", b"UI", b"EF", b"JL")
    assert len(extra) <= len(flanks) and not set(extra) & set(b"".join(flanks)) and len(set(extra)) == len(extra)
    ref, alts = _draw_ref(seed, 800, lambda r, g: [[_snv(r, p, k)] for k in (1, 2, 3)] +
                          [[("snv", p - 1, flanks[j][0]), ("snv", p, x), ("snv", p + 1, flanks[j][1])] for j, x in enumerate(extra)])
    size = 4 + len(extra)
    return Window(f"ring_{size}", [Comp(ref, alts)], claims=(max(4, 1 + len(extra)), max(4, 1 + len(extra)), size), n_alleles=size - 1)


def _long_insertions(name, n_alts, ins_len, seed, n=1000):
    """n_alts ALT haplotypes with one insertion of ins_len bases each, 60 bases apart"""
    ref, alts = _draw_ref(seed, n, lambda r, g: [[("ins", 50 + 60 * i, rand_dna(g, ins_len))] for i in range(n_alts)])
    return Window(name, [Comp(ref, alts)])


# what ma_last_poa_retry reports for a group: windows marked for the width, for the capacity only, and left flagged
MARKS = {"degree8": (4, 0, 2), "ring9": (2, 0, 1), "nodes": (0, 2, 1), "both": (2, 0, 0)}


@lru_cache(maxsize=None)
def groups():
    gs = []
    small = dict(min_k=25, max_k=25, max_haps=16, max_vars=128, max_alts=8, max_allele_bytes=4096)
    gs.append(Group("degree8", capi.default_params(**small), _interleave(
        [_plain("degree8_plain_a", 7020), _out_degree(3, 7003), _plain("degree8_plain_b", 7021), _in_degree(3, 7013), _plain("degree8_plain_c", 7022)],
        # (seeds for which _draw_ref finds a REF within its tries: thirteen bases without a repeat and sixteen unequal pairs)
        [_retag(_out_degree(7, 7004), True), _retag(_out_degree(8, 7039), False),
         _retag(_in_degree(7, 7001), True), _retag(_in_degree(8, 7003), False)]), routes=False))
    gs.append(Group("ring9", capi.default_params(**dict(small, max_alts=12)), _interleave(
        [_plain("ring9_plain_a", 7120), _ring(b"", 7100), _plain("ring9_plain_b", 7121)],
        [_retag(_ring_n(b"Nacgt", 7109), True), _retag(_ring_n(b"Nacgtn", 7110), False)]), routes=False))
    gs.append(Group("nodes", capi.default_params(**small), _interleave(
        [_insertions("nodes_ins_2x60", 2, 7200), _plain("nodes_plain_a", 7220, 900), _plain("nodes_plain_b", 7221, 950)],
        [_retag(_long_insertions("ins_12x60", 12, 60, 7212), True), _retag(_long_insertions("ins_15x120", 15, 120, 7215), False)]), routes=False))
    over_w, over_n = _out_degree(5, 7300).comps[0], _insertions("unused", 8, 7301).comps[0]
    fit_a, capped, fit_c = _out_degree(2, 7310).comps[0], _in_degree(5, 7311).comps[0], _ring(b"N", 7312).comps[0]
    over_n.anchor, capped.anchor, fit_c.anchor = ANCHOR + 1000, ANCHOR + 1000, ANCHOR + 2000
    gs.append(Group("both", capi.default_params(**small), _interleave(
        [_plain("both_plain_a", 7320), _plain("both_plain_b", 7321), _plain("both_plain_c", 7322)],
        [Window("width_then_nodes", [over_w, over_n], kind="fit"),
         Window("capped_between_two_fitting", [fit_a, capped, fit_c], kind="fit")]), routes=False))
    return {g.name: g for g in gs}


def build(group):
    """-> (arrs, n, nr, asm) of a group, like poa_cases.build"""
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
