"""Batches for the packed-read tests (tests/test_packed_reads.py, tests/test_gpu_packed_reads.py): synth windows with reads
cut to odd lengths, one window without reads, every one of BAM's sixteen base letters somewhere, and qualities either
quantised to 8 levels (the 4-bit dictionary) or left raw (8-bit)."""
import functools

import numpy as np

from lancet2_amd import capi, synth

LETTERS = np.frombuffer(capi.BASE_CODES.encode(), dtype=np.uint8)
CASES = {"C2": 8, "C5": 4}  # synth configuration -> windows


def params(cfg):
    return capi.default_params(min_k=25, max_k=25, num_samples=3 if cfg == "C5" else 2)


@functools.lru_cache(maxsize=None)
def _windows(cfg):
    n = CASES[cfg]
    kw = dict(synth.CONFIGS[cfg])
    wins = [synth.make_window(700 + i, **kw) for i in range(n)]
    rng = np.random.default_rng(77)
    wins[2]["reads"] = []  # a window with no reads (in the first lane's slice of a two-lane run; the second starts after it)
    cuts = (149, 143, 9, 8, 7, 2, 1, 151)
    for wi, w in enumerate(wins):
        for ri, r in enumerate(w["reads"]):
            if (ri + wi) % 5 == 0:  # odd lengths, short reads, offsets of every parity
                ln = cuts[(ri // 5 + wi) % len(cuts)]
                if ln <= len(r["seq"]):
                    r["seq"], r["qual"] = r["seq"][:ln].copy(), r["qual"][:ln].copy()
                else:
                    r["seq"] = np.concatenate([r["seq"], r["seq"][:ln - len(r["seq"])]])
                    r["qual"] = np.concatenate([r["qual"], r["qual"][:ln - len(r["qual"])]])
            if ri % 11 == 3 and len(r["seq"]) > 20:  # every letter of the code table, a few times per window
                r["seq"] = r["seq"].copy()
                at = rng.integers(0, len(r["seq"]), 2)
                r["seq"][at] = LETTERS[(ri // 11 + np.arange(2) * 7 + wi) % 16]
    return wins


@functools.lru_cache(maxsize=None)
def batch(cfg, qual_bits):
    """-> (arrs, n, nr, packed, twin): twin = the ASCII arrays the device decodes, packed = capi.pack_reads' dict"""
    arrs, n, nr = synth.pack_batch(_windows(cfg))
    total = int(arrs["read_off"][-1])
    seen = set(np.unique(arrs["read_bases"][:total]).tolist())
    assert seen == set(LETTERS.tolist()), sorted(seen)
    assert int(arrs["read_win_off"][3]) == int(arrs["read_win_off"][2])
    assert np.any((arrs["read_off"][1:] - arrs["read_off"][:-1]) % 2 == 1)
    if qual_bits == 4:
        arrs["read_quals"] = (np.minimum(arrs["read_quals"], 41) // 6 * 6).astype(np.uint8)  # 8 levels: 0, 6, ... 36 (and 42 never)
        assert len(np.unique(arrs["read_quals"][:total])) <= 16
    packed, twin = capi.pack_reads(arrs)
    assert packed["qual_bits"] == qual_bits, (packed["qual_bits"], len(np.unique(arrs["read_quals"][:total])))
    assert np.array_equal(twin["read_bases"], arrs["read_bases"]) and np.array_equal(twin["read_quals"], arrs["read_quals"])
    return arrs, n, nr, packed, twin
