"""No GPU: the inputs of tests/test_gpu_general_deferral.py are what its cases need.  Distinct canonical k-mers per window are
counted on the CPU against the 6144 entries of k_insert's LDS map (= the largest table k_graph takes): a window above it needs
the general table route, a window below ~5000 does not come near it.  An N-containing k-mer adds at most one table entry and
a headline window holds at most 581 of them, which the counts leave out: "large" therefore means more than 6144 + 581 over
the reads that pass the filter alone, "small" less than 5000 over all reads."""
import numpy as np

import deferral_cases as dc
from lancet2_amd import capi, synth

BIG = dc.MAP_ENTRIES + dc.N_PER_WINDOW_MAX
SMALL = 5000


def test_headline_windows_stay_below_the_map():
    wins = dc.headline_windows(64)
    counts = [dc.distinct_kmers(w) for w in wins]
    assert max(counts) < SMALL, counts
    ok, why = dc.mode_available(wins, dc.K)
    assert ok, why


def test_mixed_batch_has_both_groups_and_keeps_the_mode():
    wins = dc.mixed_windows()
    big = [dc.distinct_kmers(wins[i], pass_only=True) for i in dc.BIG_AT]
    small = [dc.distinct_kmers(w) for i, w in enumerate(wins) if i not in dc.BIG_AT]
    assert len(big) in (2, 3) and min(big) > BIG, big
    assert len(small) >= 12 and max(small) < SMALL, small
    assert 256 * len(big) > len(wins)  # (more than 1 window in 256: the batch that switches a context off)
    ok, why = dc.mode_available(wins, dc.K)
    assert ok and why["lds"] < dc.GRAPH_LDS_LIMIT * 3 // 4 and why["max_reads"] + 1 < dc.SEQ_CAP // 2, why


def test_support_group_batch_has_names_in_two_runs_and_keeps_the_mode():
    wins, two_runs = dc.support_group_windows()
    assert len(two_runs) >= 2
    for i in two_runs:
        keys = [(r["qname"], r["role"]) for r in wins[i]["reads"] if r["passf"]]
        runs = 1 + sum(a != b for a, b in zip(keys, keys[1:]))
        assert runs > len(set(keys)), (i, runs, len(set(keys)))  # a key of the passing reads in two separate runs
    sizes = {}
    for r in wins[2]["reads"]:
        sizes[(r["qname"], r["role"])] = sizes.get((r["qname"], r["role"]), 0) + 1
    assert max(sizes.values()) >= 3  # a group of three reads with one name
    assert max(dc.distinct_kmers(w) for w in wins) < SMALL
    assert all(r["hint"] != capi.MA_NO_HINT for w in wins for r in w["reads"])
    ok, why = dc.mode_available(wins, dc.K)
    assert ok, why


def test_ladder_batch_outgrows_the_map_on_upper_rungs_only():
    wins = dc.ladder_windows()
    first = [dc.distinct_kmers(w, 13) for w in wins]
    assert max(first) < dc.MAP_ENTRIES - dc.N_PER_WINDOW_MAX, first  # the first rung fits, N k-mers included
    climbers = [i for i, d in enumerate(dc.LADDER_DUPS) if d]
    upper = [dc.distinct_kmers(wins[i], 61, pass_only=True) for i in climbers]  # (61 = 13 + 8 x 6: a rung above every duplication but the 80s')
    assert min(upper) > BIG, upper
    rest = [dc.distinct_kmers(w, 61) for i, w in enumerate(wins) if i not in climbers]
    assert max(rest) < dc.MAP_ENTRIES - dc.N_PER_WINDOW_MAX, rest
    ok, why = dc.mode_available(wins, 13)
    assert ok, why


def test_small_and_gated_batches():
    a, s = dc.mixed_windows(), dc.small_windows()
    assert len(s) == 4 and max(len(w["reads"]) for w in s) < min(len(w["reads"]) for w in a)
    g = dc.gated_windows()
    for w in g:  # the reference itself repeats 200 bases: a repeat longer than k = 25
        ref = w["ref"].tobytes()
        assert any(ref.find(ref[i:i + 100], i + 1) > 0 for i in range(0, len(ref) - 100, 10))
    arrs, n, nr = synth.pack_batch(g)
    assert n == 4 and nr > 0 and np.all(arrs["read_hint"] != capi.MA_NO_HINT)
