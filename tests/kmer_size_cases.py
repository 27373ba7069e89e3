"""The case table of the k-mer size sweep (inputs only: generator arguments and seeds, nothing from oracle/).

tests/test_gpu_kmer_sizes.py runs the engine and the oracle over it; tests/test_kmer_size_cases.py runs the oracle alone
and asserts the non-vacuity floor, so that the floor is checked without a GPU and an edit of synth.py cannot quietly empty
the sweep."""
import numpy as np

from lancet2_amd import capi, synth

# small k | the 2-bit packing boundary (k <= 32 packs into one word) | two and three 64-bit words of bases | up to the default
# top of the ladder
SWEEP_KS = (13, 15, 17, 19, 21, 23, 27, 29, 31, 33, 35, 47, 49, 61, 63, 65, 67, 79, 95, 97, 99, 111, 125, 127)
# above the default max_k, up to the reference's hard bound (cbdg/graph_params.h:15)
HIGH_KS = (129, 191, 255)
ROUTE_KS = (31, 33, 65, 127)


def _window_len(K):
    """The default repeat gate (max_mismatch = 2) skips most random 1001-base windows at k = 13 and 15: P(two k-mers within
    two mismatches) is 1.1e-5 at k = 13 and 9e-7 at k = 15, times W^2 / 2 pairs.  Shorter windows keep the gate open.
    Above 127 the window has to hold the longer anchors and reads."""
    if K <= 13:
        return 300
    if K <= 15:
        return 450
    if K <= 17:
        return 700
    return 1001 if K <= 127 else 1301


def _read_len(K):
    """250-base reads above 127; at 255 a 250-base read has no k-mer at all, so 400 (the genotyper takes reads up to 608)"""
    return 150 if K <= 127 else 250 if K < 250 else 400


def lower_case_some_reads(win, seed, frac=0.12):
    """soft-masked stretches: in `frac` of the window's reads 4 to 40 bases become lower case (in place; returns win)"""
    rng = np.random.default_rng(seed)
    for r in win["reads"]:
        if rng.random() < frac:
            n = len(r["seq"])
            ln = int(rng.integers(4, 41))
            at = int(rng.integers(0, max(1, n - ln)))
            seg = r["seq"][at:at + ln]
            acgt = np.isin(seg, synth.BASES)
            seg[acgt] |= 0x20
    return win


def first_index(K):
    return 110_000 + 100 * K


def sweep_params(K, **kw):
    pk = dict(min_k=K, max_k=K)
    if K > 127:
        pk["max_hap_len"] = 4096
    pk.update(kw)
    return capi.default_params(**pk)


_DEEP_FROM = 95  # a heterozygous variant's k-mers are seen (read_len - k + 1) / read_len as often as its bases: 37 % at k = 95
_C5_FIRST = {99: 23, 125: 24, 127: 24}  # three-sample windows that hold a variant the oracle can still assemble at this k


def main_windows(K):
    """The mixed two-sample batch of one K: plain C2, C3 with soft clips and N (their reads are not staged in LDS, the
    others' are), an STR, lower-case stretches, a short C1 window, and noisy reads with more indels or -- from K = 97 up --
    250-base reads (a 150-base read has 54 k-mers at k = 97 and 24 at k = 127)."""
    W, RL, f = _window_len(K), _read_len(K), first_index(K)
    c2 = dict(synth.CONFIGS["C2"], W=W, read_len=RL)
    c3 = dict(synth.CONFIGS["C3"], W=W, read_len=RL)
    if K >= _DEEP_FROM:
        c2["depths"] = (60, 60)
        c3["depths"] = (60, 90)
    eighth = dict(c2, read_len=250) if K >= 97 else dict(c2, error_scale=3.0, indel_rate=1e-3)
    wins = [synth.make_window(f + 0, **c2),
            synth.make_window(f + 3, softclip_frac=0.08, n_frac=0.05, **c3),
            synth.make_window(f + 5, str_unit=b"CAG", n_somatic=2, **c2),
            lower_case_some_reads(synth.make_window(f + 6, **c2), seed=f + 6),
            synth.make_window(f + 8, **eighth),
            synth.make_window(f + 9, **dict(c2, W=min(W, 600))),
            synth.make_window(f + 1, **c2),
            synth.make_window(f + 4, softclip_frac=0.05, n_frac=0.10, **c3)]
    return wins


def three_sample_windows(K):
    W, RL, f = _window_len(K), _read_len(K), first_index(K) + _C5_FIRST.get(K, 20)
    c5 = dict(synth.CONFIGS["C5"], W=W, read_len=RL)
    if K >= _DEEP_FROM:
        c5["depths"] = (60, 60, 60)
    return [synth.make_window(f, **c5), synth.make_window(f + 1, n_frac=0.05, **c5)]


def sweep_batches(K):
    """-> [(name, params, arrs, n, nr)]: the mixed batch and the small three-sample batch of one K"""
    out = []
    for name, wins, kw in (("mixed", main_windows(K), {}), ("three samples", three_sample_windows(K), dict(num_samples=3))):
        arrs, n, nr = synth.pack_batch(wins)
        out.append((name, sweep_params(K, **kw), arrs, n, nr))
    return out


def floor_of(K, asm, var, n):
    """The non-vacuity floor on ORACLE output: -> (assembled windows, windows with a component of >= 2 haplotypes,
    variants, list of violations)."""
    MC = asm["comp_nhaps"].size // asm["win_ncomp"].size
    ncomp = asm["win_ncomp"][:n].astype(np.int64)
    assembled = ncomp > 0
    multi = np.array([bool(ncomp[w]) and int(asm["comp_nhaps"][w * MC:w * MC + ncomp[w]].max()) >= 2 for w in range(n)])
    nvars = int(var["win_nvars"][:n].sum()) if var is not None else -1
    bad = []
    if 2 * int(multi.sum()) < n:
        bad.append(f"k={K}: {int(multi.sum())} of {n} windows have a component with >= 2 haplotypes")
    if var is not None and nvars < 1:
        bad.append(f"k={K}: no variant")
    if not (asm["win_k"][:n][assembled] == K).all():
        bad.append(f"k={K}: win_k {asm['win_k'][:n].tolist()}")
    return int(assembled.sum()), int(multi.sum()), nvars, bad
