"""Inputs for the POA export tests (tests/test_poa_graph_ref.py, tests/test_gpu_poa_export.py): seeded components of a REF
haplotype and ALT haplotypes with substitutions, insertions and deletions.  Inputs only -- nothing here looks at the engine,
the oracle or the restatement."""
import numpy as np

from pin_cases import rand_dna

BASES = b"ACGT"


def mutated(rng, ref, n_snv, n_ins, n_del, max_indel=12):
    """ref with n_snv substitutions, n_ins insertions and n_del deletions of 1 .. max_indel bases at random places"""
    b = bytearray(ref)
    for _ in range(n_snv):
        i = int(rng.integers(0, len(b)))
        b[i] = BASES[(BASES.index(bytes([b[i]])) + int(rng.integers(1, 4))) % 4]
    for _ in range(n_ins):
        i = int(rng.integers(0, len(b) + 1))
        b[i:i] = rand_dna(rng, int(rng.integers(1, max_indel + 1)))
    for _ in range(n_del):
        L = int(rng.integers(1, max_indel + 1))
        if len(b) > L + 2:
            i = int(rng.integers(0, len(b) - L))
            del b[i:i + L]
    return bytes(b)


def random_component(rng, lo=30, hi=400, min_haps=2, max_haps=9):
    """a REF of lo .. hi bases and 1 .. max_haps - 1 ALT haplotypes, each with up to three edits of every kind"""
    ref = rand_dna(rng, int(rng.integers(lo, hi + 1)))
    nh = int(rng.integers(min_haps, max_haps + 1))
    haps = [ref]
    for _ in range(nh - 1):
        h = mutated(rng, ref, int(rng.integers(0, 4)), int(rng.integers(0, 3)), int(rng.integers(0, 3)))
        haps.append(h[:hi] if len(h) > hi else h)
    return haps


def seeded_components(count=40, seed=20261020):
    rng = np.random.default_rng(seed)
    return [random_component(rng) for _ in range(count)]
