"""Developer tool: the extract stage with and without --raw-records, on the input `also.pipeline_extract`
of bench.py is quoted on -- a random 2.4 Mb genome, 60x / 30x, 150-base pairs, plain 150M alignments -- written as BAM (no
index: the files are read whole).  Builds examples/pipeline_driver.cpp -O3 -march=native as bench.py does, and, with
--parent-src DIR (a checkout of another commit: DIR/examples, DIR/include, DIR/lancet2_amd/host), that commit's driver too;
runs `--extract-only --no-active-region` with 1 and N collector threads, three times each, and prints windows/s handed over and
cpu-seconds of collection per window (median and the three runs).
With --active-region the reads carry a planted SNV every 700 bases (sequence bytes and MD strings say so), the runs leave
active-region detection ON, and a third leg runs `--raw-records --device-select`: the collector lists every candidate and looks
at none -- the filters, the detection and the coverage gates are the engine's (ma_select_records_batch).
usage: python tools/extract_cost.py [--parent-src DIR] [--threads N] [--genome-len L] [--active-region]"""
import argparse
import os
import re
import statistics
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_bam(path, genome, name, depth, rng, snv_every=0):
    """coordinate-sorted BAM of genome_len * depth / 300 pairs; returns the number of records"""
    glen = len(genome)
    code = np.zeros(256, np.uint8)
    for i, ch in enumerate(b"=ACMGRSVTWYHKDBN"):
        code[ch] = i
    c = code[genome]
    even = bytes(((c[0:glen - 1:2] << 4) | c[1:glen:2]).astype(np.uint8))   # byte k: bases 2k, 2k + 1
    odd = bytes(((c[1:glen - 1:2] << 4) | c[2:glen:2]).astype(np.uint8))    # byte k: bases 2k + 1, 2k + 2
    npairs = glen * depth // 300
    starts = np.sort(rng.integers(0, glen - 550, npairs))
    recs = []
    for i, s0 in enumerate(starts):
        s1 = int(s0) + 250 + int(rng.integers(0, 150))
        recs.append((int(s0), i, 0x63, s1))
        recs.append((s1, i, 0x93, int(s0)))
    recs.sort()
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n" % glen
    out = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" +
                    struct.pack("<i", glen))
    qual, cigar, tag = b"\x28" * 150, struct.pack("<I", (150 << 4) | 0), b"MDZ150\0"
    for pos0, i, flag, mate in recs:
        qn = b"%c%d\0" % (name[0].encode(), i)
        seq = (even if pos0 % 2 == 0 else odd)[pos0 // 2:pos0 // 2 + 75]
        tag = b"MDZ150\0"
        site = -(-pos0 // snv_every) * snv_every if snv_every else glen
        if site < pos0 + 150:  # the planted SNV: the next base code in the read, the reference's letter in the MD string
            at = site - pos0
            was = int(c[site])
            now = {1: 2, 2: 4, 4: 8, 8: 1}[was]
            seq = bytearray(seq)
            seq[at // 2] = (seq[at // 2] & (0x0F if at % 2 == 0 else 0xF0)) | (now << (4 if at % 2 == 0 else 0))
            seq = bytes(seq)
            tag = b"MDZ%d%c%d\0" % (at, genome[site], 149 - at)
        body = struct.pack("<iiBBHHHiiii", 0, pos0, len(qn), 60, 4680, 1, flag, 150, 0, mate, mate - pos0) + qn + cigar + seq + qual + tag
        out += struct.pack("<i", len(body)) + body
    with open(path, "wb") as fh:
        for at in list(range(0, len(out), 60000)) + [None]:
            data = bytes(out[at:at + 60000]) if at is not None else b""
            comp = zlib.compressobj(1, zlib.DEFLATED, -15)
            cdata = comp.compress(data) + comp.flush()
            fh.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(cdata) + 25) + cdata +
                     struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))
    return len(recs)


def build_driver(src_root, exe):
    lib = os.path.join(REPO, "lancet2_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-march=native", os.path.join(src_root, "examples", "pipeline_driver.cpp"), "-I",
                           os.path.join(src_root, "include"), "-L", lib, "-lmicroasm", f"-Wl,-rpath,{lib}", "-Wl,--allow-shlib-undefined",
                           "-DLANCET2_AMD_WITH_ZLIB", "-lz", "-lpthread", "-o", exe])


def run(exe, d, mode, nthreads, active_region=False):
    r = subprocess.run([exe, "--reference", os.path.join(d, "ref.fa"), "--normal", os.path.join(d, "normal.bam"), "--tumor",
                        os.path.join(d, "tumor.bam"), "--extract-only", "--extract-threads", str(nthreads)] +
                       ([] if active_region else ["--no-active-region"]) + mode.split(), capture_output=True, text=True)
    m = re.search(r"extract ([0-9.]+) s busy \(([0-9.]+) windows/s tiled, ([0-9.]+) shipped/s\) with (\d+) collector thread\(s\), ([0-9.]+) cpu-s of collection", r.stderr)
    if r.returncode != 0 or not m:
        raise RuntimeError(f"{exe} {mode}: " + r.stderr[-300:])
    nwin = int(re.search(r"pipeline_driver: (\d+) windows", r.stderr).group(1))
    return float(m.group(3)), float(m.group(5)) / nwin * 1e6, nwin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-src")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--genome-len", type=int, default=2_400_000)
    ap.add_argument("--active-region", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="ma_extract_") as d:
        rng = np.random.default_rng(0x5EED)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, args.genome_len)]
        with open(os.path.join(d, "ref.fa"), "w") as f:
            f.write(">chr1\n" + bytes(genome).decode() + "\n")
        nrec = sum(write_bam(os.path.join(d, name + ".bam"), genome, name, depth, rng, 700 if args.active_region else 0)
                   for name, depth in (("normal", 30), ("tumor", 60)))
        legs = []
        if args.parent_src:
            build_driver(args.parent_src, os.path.join(d, "driver_parent"))
            legs.append(("parent --raw-records" if args.active_region else "parent --packed-reads", os.path.join(d, "driver_parent"),
                         "--raw-records" if args.active_region else "--packed-reads"))
        build_driver(REPO, os.path.join(d, "driver"))
        legs += [("this --packed-reads", os.path.join(d, "driver"), "--packed-reads"), ("this --raw-records", os.path.join(d, "driver"), "--raw-records")]
        if args.active_region:
            legs.append(("this --raw-records --device-select", os.path.join(d, "driver"), "--raw-records --device-select"))
        print(f"{args.genome_len} bases, {nrec} records, BAM read whole; -O3 -march=native; three runs each, in turn; active-region detection "
              f"{'on, an SNV every 700 bases' if args.active_region else 'off'}")
        res = {}
        for rep in range(3):  # the legs alternate: a drift of the machine hits all of them
            for nthreads in (1, args.threads):
                for label, exe, mode in legs:
                    res.setdefault((label, nthreads), []).append(run(exe, d, mode, nthreads, args.active_region))
        for (label, nthreads), runs in res.items():
            wps, us = [r[0] for r in runs], [r[1] for r in runs]
            print(f"{label}, {nthreads} collector thread(s): {statistics.median(wps):.0f} windows/s (runs {[round(x) for x in wps]}), "
                  f"{statistics.median(us):.1f} cpu-us of collection per window (runs {[round(x, 1) for x in us]}), {runs[0][2]} windows")


if __name__ == "__main__":
    sys.exit(main())
