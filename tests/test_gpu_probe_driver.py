"""pipeline_driver --probe-variants FILE --probe-results FILE on the small genome and SAM files of tests/test_pipeline_host.py:
the probes file is made from the run's own VCF records plus one decoy, in the reference's missed_variants.txt layout; the results
file must carry the reference's header, one line per (probe, window, component row), the columns the engine produces equal to
tests/probe_ref.py on the dumped batches, and "." everywhere else."""
import os
import subprocess
import types

import numpy as np
import pytest

import probe_cases as pc
from lancet2_amd import capi
from lancet2_amd.engine import Engine

pytestmark = pytest.mark.gpu

# cbdg/probe_results_writer.cpp:51-59
HEADER = ("probe_id chrom pos ref alt window n_raw_alt_reads kmer_size n_expected_alt_kmers n_alt_kmers_in_reads comp_id n_comp_nodes "
          "n_split_across_comps n_surviving_build n_surviving_lowcov1 n_surviving_compress1 n_surviving_lowcov2 n_surviving_compress2 "
          "n_surviving_tips hap_indices is_traversal_limited is_graph_cycle is_graph_complex is_no_anchor is_short_anchor "
          "is_variant_in_anchor n_last_edge_kmers n_last_interior_kmers n_last_chain_gaps msa_shift_bp is_msa_exact_match is_msa_shifted "
          "is_msa_subsumed n_geno_true_alt_reads n_geno_total_ref_reads n_geno_reassigned_to_ref n_geno_reassigned_to_wrong_alt "
          "n_geno_non_overlapping is_geno_has_alt_support is_geno_no_overlap").split()
FILLED = {"probe_id", "chrom", "pos", "ref", "alt", "window", "n_raw_alt_reads", "kmer_size", "n_expected_alt_kmers", "n_alt_kmers_in_reads",
          "comp_id", "n_surviving_lowcov1", "n_surviving_tips", "hap_indices", "n_last_edge_kmers", "n_last_interior_kmers", "n_last_chain_gaps"}


def test_driver_writes_the_probe_records_of_every_window(tmp_path):
    from test_pipeline_host import driver, write_fixture
    exe = driver(tmp_path)
    write_fixture(str(tmp_path))
    common = [exe, "--reference", str(tmp_path / "ref.fa"), "--normal", str(tmp_path / "normal.sam"), "--tumor", str(tmp_path / "tumor.sam"),
              "--region", "chr1:1-6000", "--min-kmer", "25", "--max-kmer", "25", "--batch-windows", "3"]
    r0 = subprocess.run(common + ["--out-vcf", str(tmp_path / "plain.vcf")], capture_output=True, text=True)
    assert r0.returncode == 0, r0.stderr
    body = lambda path: [ln for ln in open(path).read().splitlines() if not ln.startswith("##commandLine=")]  # noqa: E731
    records = [ln.split("\t") for ln in body(tmp_path / "plain.vcf") if not ln.startswith("#")]
    assert records
    # missed_variants.txt: a header, then chrom, 0-based start, end, ref, alt, type, length, classification, raw_alt_count, ...
    variants = []
    for rec in records:
        for alt in rec[4].split(","):
            variants.append((rec[0], int(rec[1]) - 1, rec[3], alt, 7 + len(variants)))
    variants.append(("chr1", 3300, "A", "ACGTTGCA", 0))   # a decoy: an insertion nobody carries, where two windows overlap
    variants.append(("chr2", 100, "A", "C", 3))           # another chromosome: activated nowhere
    with open(tmp_path / "missed.txt", "w") as f:
        f.write("chrom\tstart\tend\tref\talt\ttype\tlength\tclassification\traw_alt_count\traw_total_depth\n")
        f.write("chr1\t10\t11\tA\n")                       # too few fields: skipped, takes no probe id (probe_index.cpp:167-168)
        for ch, s, ref, alt, raw in variants:
            f.write(f"{ch}\t{s}\t{s + len(ref)}\t{ref}\t{alt}\tX\t{abs(len(alt) - len(ref))}\tmissed\t{raw}\t40\n")
    dump = tmp_path / "dump"
    dump.mkdir()
    r1 = subprocess.run(common + ["--out-vcf", str(tmp_path / "probed.vcf"), "--probe-variants", str(tmp_path / "missed.txt"),
                                  "--probe-results", str(tmp_path / "results.tsv"), "--dump", str(dump)], capture_output=True, text=True)
    assert r1.returncode == 0, r1.stderr
    assert body(tmp_path / "plain.vcf") == body(tmp_path / "probed.vcf")   # a debugging mode: the calls are those of a run without it
    lines = open(tmp_path / "results.tsv").read().splitlines()
    assert lines[0].split("\t") == HEADER and len(HEADER) == 40
    got = [dict(zip(HEADER, ln.split("\t"))) for ln in lines[1:]]
    assert all(len(ln.split("\t")) == 40 for ln in lines[1:])
    assert f"{len(got)} probe records of {len(variants)} truth variants" in r1.stderr, r1.stderr

    # what the lines must be: probe_ref on the dumped batches, with the engine's own assembly rows
    params = capi.default_params(min_k=25, max_k=25)
    dt = {"u8": np.uint8, "u32": np.uint32, "u64": np.uint64, "i32": np.int32}
    want, hits = [], 0
    eng = Engine(params)
    try:
        for b in sorted(os.listdir(dump)):
            arrs = {f.rsplit(".", 1)[0]: np.fromfile(str(dump / b / f), dtype=dt[f.rsplit(".", 1)[1]]) for f in os.listdir(dump / b)}
            wins = arrs.pop("windows").reshape(-1, 4)
            n, nr = len(wins), len(arrs["read_qname_id"])
            asm = eng.assemble(arrs, n, nr)
            lists = [[(s - (int(w1) - 1), len(ref), alt.encode(), i) for i, (ch, s, ref, alt, _) in enumerate(variants)
                      if ch == "chr1" and int(w1) - 1 <= s < int(w2) and s + len(ref) <= int(w2)] for _, w1, w2, _ in wins]
            c = types.SimpleNamespace(params=params, arrs=arrs, n=n, nr=nr)
            rows = pc.expected_rows(None, asm, per_window=lists, case_obj=c)
            for w in range(n):
                region = f"chr1:{int(wins[w, 1])}-{int(wins[w, 2])}"
                ncomp = int(asm["win_ncomp"][w])
                for row, (_, _, _, i) in zip(rows[w], lists[w]):
                    ch, s, ref, alt, raw = variants[i]
                    assert row["pb_final"] is not None and row["pb_lowcov1"] is not None
                    for ci in range(max(ncomp, 1)):
                        fin = row["pb_final"][4 * ci:4 * ci + 4]
                        haps = ",".join(str(h) for h in range(32) if row["pb_hap_mask"][ci] >> h & 1) if ncomp else ""
                        hits += bool(haps)
                        exp = dict(probe_id=str(i), chrom=ch, pos=str(s), ref=ref, alt=alt, window=region, n_raw_alt_reads=str(raw),
                                   kmer_size=str(row["pb_k"]), n_expected_alt_kmers=str(row["pb_alt_kmers"]),
                                   n_alt_kmers_in_reads=str(row["pb_in_reads"][0]), comp_id=str(ci) if ncomp else ".",
                                   n_surviving_lowcov1=str(row["pb_lowcov1"][0]), n_surviving_tips=str(fin[0]) if ncomp else ".",
                                   hap_indices=haps or ".", n_last_edge_kmers=str(fin[1]) if ncomp else ".",
                                   n_last_interior_kmers=str(fin[2]) if ncomp else ".", n_last_chain_gaps=str(fin[3]) if ncomp else ".")
                        exp.update({k: "." for k in HEADER if k not in FILLED})
                        want.append(exp)
    finally:
        eng.close()
    assert len(got) == len(want), (len(got), len(want))
    for g, x in zip(got, want):
        assert g == x, {k: (g[k], x[k]) for k in HEADER if g[k] != x[k]}
    # the run's own records are found in a haplotype somewhere, the decoy nowhere; windows overlap: some variant has two lines
    decoy = [g for g in got if g["probe_id"] == str(len(variants) - 2)]
    assert 2 * hits >= len(records) and decoy and all(g["hap_indices"] == "." and g["n_alt_kmers_in_reads"] == "0" for g in decoy)
    assert len(decoy) >= 2 and not any(g["chrom"] == "chr2" for g in got)
    # the flags go together
    r2 = subprocess.run(common + ["--probe-variants", str(tmp_path / "missed.txt")], capture_output=True, text=True)
    assert r2.returncode == 2 and "go together" in r2.stderr
