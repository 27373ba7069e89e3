"""Inputs of tests/test_gpu_general_deferral.py and the CPU-side facts about them that tests/test_general_deferral_inputs.py
asserts without a GPU: how many distinct canonical k-mers a window holds (against the 6144 entries of k_insert's LDS map and of
the tables k_graph takes), and whether the batch keeps the common-route-only pass of the build stage available (k_graph's LDS
footprint within its limit, no window of more sequences than a queued key names)."""
import numpy as np

from lancet2_amd import capi, synth

K = 25
MAP_ENTRIES = 6144      # build.hip: kInsMapA == kGrSlots
SEQ_CAP = 2048          # build.hip: kSeqCap
GRAPH_LDS_LIMIT = 120 * 1024
N_PER_WINDOW_MAX = 581  # most N-containing k-mers of a headline window (each adds at most one table entry)

_CODE = np.full(256, -1, np.int64)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def _canonical_kmers(seq, k):
    """the canonical k-mers of `seq` that hold no N, as python ints (k <= 31) or bytes"""
    if len(seq) < k:
        return set()
    c = _CODE[np.asarray(seq, np.uint8)]
    win = np.lib.stride_tricks.sliding_window_view(c, k)
    ok = (win >= 0).all(axis=1)
    win = win[ok]
    if not len(win):
        return set()
    if k <= 31:
        pw = (np.uint64(4) ** np.arange(k - 1, -1, -1, dtype=np.uint64))
        fwd = (win.astype(np.uint64) * pw).sum(axis=1, dtype=np.uint64)
        rc = ((3 - win[:, ::-1]).astype(np.uint64) * pw).sum(axis=1, dtype=np.uint64)
        return set(np.minimum(fwd, rc).tolist())
    f = win.astype(np.uint8)
    r = (3 - win[:, ::-1]).astype(np.uint8)
    return {min(a.tobytes(), b.tobytes()) for a, b in zip(f, r)}


def distinct_kmers(win, k=K, pass_only=False):
    """distinct canonical k-mers of the window's reference and reads (pass_only: of the reads that pass the filter only)"""
    s = _canonical_kmers(win["ref"], k)
    for r in win["reads"]:
        if pass_only and not r["passf"]:
            continue
        s |= _canonical_kmers(r["seq"], k)
    return len(s)


def graph_lds_bytes(inst_stride, ref_stride, S):
    """build.hip: graph_lds_bytes / graph_area_bytes"""
    nw = (inst_stride + 31) // 32 + 1
    area = max(4 * nw + 2 * nw + 4 * SEQ_CAP + 64, 8 * MAP_ENTRIES, 2 * MAP_ENTRIES * (S + 2))
    area = (area + 15) & ~15
    return 2 * MAP_ENTRIES + MAP_ENTRIES // 8 + ((2 * ref_stride + 15) & ~15) + area + 64


def mode_available(wins, k, S=2):
    """what run_build_pass decides from the batch's maxima (assemble.hip: inst_stride, ref_stride, max_reads at min_k)"""
    max_inst = max(sum(max(0, len(s) - k + 1) for s in [w["ref"]] + [r["seq"] for r in w["reads"]]) for w in wins)
    max_refk = max(len(w["ref"]) - k + 1 for w in wins)
    max_reads = max(len(w["reads"]) for w in wins)
    lds = graph_lds_bytes((max_inst + 63) & ~63, (max_refk + 63) & ~63, S)
    return lds <= GRAPH_LDS_LIMIT and max_reads + 1 <= SEQ_CAP, dict(lds=lds, max_reads=max_reads, max_inst=max_inst)


def headline_windows(count=64, first=10000):
    """the benchmark's own C3 windows (bench.window_kwargs: short tandem repeats, tandem duplications, low complexity, soft
    clips, N bases, every 50th name without a hint)"""
    import bench
    wins = []
    for idx in range(first, first + count):
        w = synth.make_window(idx, **bench.window_kwargs("C3", idx, 8))
        for r in w["reads"]:
            if r["qname"] % 50 == 49:
                r["hint"] = capi.MA_NO_HINT
        wins.append(w)
    return wins


BIG_AT = (3, 9, 14)  # windows of the mixed batch whose reads carry eight times the sequencing errors


def mixed_windows(first=171_000, n=16, big_at=BIG_AT, k=K):
    """ordinary C3 windows, and at `big_at` windows that outgrow the 6144-entry map: every read error adds up to k distinct
    k-mers"""
    c3 = synth.CONFIGS["C3"]
    return [synth.make_window(first + i, **dict(c3, **({"error_scale": 8.0} if i in big_at else {}))) for i in range(n)]


LADDER_DUPS = (0, 60, 0, 80, 45, 0, 80, 60)  # tandem duplication of the ladder batch's windows (0: none)


def ladder_windows(first=172_000, n=8):
    """k = 13 ... 127: tandem duplications send windows up the ladder, and four times the sequencing errors make the climbers'
    upper rungs outgrow the map (a read error costs up to k distinct k-mers: ~5.1 k per window at 13, ~9 k at 61)"""
    c2 = synth.CONFIGS["C2"]
    return [synth.make_window(first + i, **dict(c2, **({"tandem_dup": d, "error_scale": 4.0} if d else {})))
            for i, d in zip(range(n), LADDER_DUPS)]


def support_group_windows(first=173_000):
    """windows whose mate-mer support needs a general kernel beside ordinary ones: one (qname, role) in two separate runs of
    reads (every group of the window becomes generic), and runs of three and four reads of one name (generic groups)"""
    import test_gpu_support_groups as sg
    wins = [sg._c1(first + 0), sg._two_runs_window(first + 1), sg._shape_window(first + 2, 1, 1), sg._c1(first + 3),
            sg._boundary_window(first + 4, 0, 0), sg._two_runs_window(first + 5), sg._c1(first + 6), sg._overlap_window(first + 7, 1, 1)]
    return wins, (1, 5)  # ... and the windows with a name in two runs


def small_windows(first=174_000, n=4):
    """fewer and shallower windows than any other batch here (what runs between two calls on a larger batch)"""
    return [synth.make_window(first + i, **dict(synth.CONFIGS["C1"], depths=(12, 12))) for i in range(n)]


def gated_windows(first=175_000, n=4):
    """windows the repeat gate stops at the one k attempted: a dispersed duplication of the reference longer than k -- no window
    is assembled, the POA and genotype stages run on nothing"""
    return [synth.make_window(first + i, **dict(synth.CONFIGS["C2"], dup_len=200)) for i in range(n)]
