"""ma_assemble_probe_batch against tests/probe_ref.py: every row the engine returns for a probe -- k, the ALT-unique k-mers,
their occurrences in the reads, the profiles after the first low-coverage pass and in every pruned component, the haplotypes
that spell the allele -- must equal, exactly, what a plain restatement of the definitions in include/microasm.h makes of the
batch's bytes and the call's own assembly rows, on the cases of tests/probe_cases.py and on the three clean routes.
tests/test_probe_cases.py shows without a GPU that the restatement is right on a toy worked out by hand and that the cases
reach their edges."""
import ctypes as C

import numpy as np
import pytest

import probe_cases as pc
from lancet2_amd import capi
from lancet2_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

ROUTE_ENVS = {"compact": {}, "raw": {"MA_NO_CHAINS": "1"}, "large classes": {"MA_CHAINS_CAP": "64"}, "no fuse": {"MA_NO_GRAPH_FUSE": "1"}}
RUNS = [("handmade", r) for r in ROUTE_ENVS] + [("c2", r) for r in ("compact", "raw", "large classes")] + \
       [("c3_ladder", "compact"), ("c5_three_samples", "compact"), ("gap", "compact"), ("edges", "compact")]
ENV_KEYS = ("MA_NO_CHAINS", "MA_CHAINS_CAP", "MA_NO_SPEC", "MA_NO_GRAPH_FUSE", "MA_ARENA_CAP", "MA_NO_CAP_RETRY")
ASM_KEYS = tuple(capi.asm_out_spec(capi.default_params(), 1))
PROBE_KERNELS = {"k_probe_raw", "k_probe_nodes", "k_probe_reads"}


def _set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run(name, lists=None, plain=False):
    """(asm, probe_out, kernel names) of Engine.assemble_probes on a case; plain: Engine.assemble"""
    c = pc.case(name)
    eng = Engine(c.params)
    try:
        if plain:
            asm, po = eng.assemble(c.arrs, c.n, c.nr), None
        else:
            asm, po = eng.assemble_probes(c.arrs, c.n, c.nr, pc.packed(name, lists))
        return asm, po, {k for k, _ in eng.kernel_times()}
    finally:
        eng.close()


def assert_same_assembly(p, a, b, n):
    """every assembly array equal byte for byte in what the call defines (the host route's staging buffers are not cleared:
    hap_bases behind hap_len and hap_runs behind hap_nruns hold whatever the allocation held)"""
    for k in ASM_KEYS:
        if k not in ("hap_bases", "hap_runs"):
            assert a[k].tobytes() == b[k].tobytes(), k
    ML, MR = p.max_hap_len, p.max_runs
    for h in range(n * p.max_haps):
        ln, nr_ = int(a["hap_len"][h]), int(a["hap_nruns"][h])
        assert a["hap_bases"][h * ML:h * ML + ln].tobytes() == b["hap_bases"][h * ML:h * ML + ln].tobytes(), ("hap_bases", h)
        assert a["hap_runs"][h * MR * 2:(h * MR + nr_) * 2].tobytes() == b["hap_runs"][h * MR * 2:(h * MR + nr_) * 2].tobytes(), ("hap_runs", h)


@pytest.mark.parametrize("name,route", RUNS)
def test_rows_are_the_restatements(name, route, monkeypatch):
    _set_env(monkeypatch, ROUTE_ENVS[route])
    c = pc.case(name)
    asm, po, names = run(name)
    assert PROBE_KERNELS <= names and "k_graph_export" not in names, names
    got, want = pc.engine_rows(name, po), pc.expected_rows(name, asm)
    bad = pc.compare_case(name, got, want)
    lists = pc.probes(name)
    n_final = sum(1 for w in range(c.n) for r in want[w] if r["pb_final"] is not None and r["pb_k"])
    print(f"{name} [{route}]: {sum(len(x) for x in lists)} probes, {n_final} with a comparable graph, k {sorted({int(k) for k in asm['win_k']})}, "
          f"{sum(1 for w in range(c.n) for r in got[w] if any(r['pb_hap_mask']))} in a haplotype: {len(bad)} differences")
    assert not bad, "\n".join(bad[:12])
    assert 2 * n_final >= sum(len(x) for x in lists)
    if route == "compact":  # the assembly is the plain call's
        plain, _, plain_names = run(name, plain=True)
        assert_same_assembly(c.params, plain, asm, c.n)
        assert not plain_names & PROBE_KERNELS
    if name == "edges":
        # the window without reads was attempted and found nothing anywhere; the window without probes shifts no row
        assert got[1] and all(not any(r["pb_in_reads"] + r["pb_lowcov1"] + r["pb_final"] + r["pb_hap_mask"]) for r in got[1])
        # (windows 0 and 3 are one window; their lists differ in the drawn bases of the absent insertion only)
        same = [i for i, (p, q) in enumerate(zip(lists[0], lists[3])) if p == q]
        assert lists[2] == [] and len(same) == len(lists[0]) - 1 and all(got[0][i] == got[3][i] for i in same)
        assert got[0][-1]["pb_lowcov1"] == [20, 2, 18, 1]


def test_a_batch_without_probes(monkeypatch):
    _set_env(monkeypatch, {})
    c = pc.case("gap")
    asm, po, names = run("gap", lists=[[]])
    assert all(v.size == 0 for v in po.values())
    plain, _, _ = run("gap", plain=True)
    assert_same_assembly(c.params, plain, asm, c.n)


def test_device_pointers_keep_their_guards_and_the_kernel_checks_the_probes(monkeypatch):
    from harness import DeviceArena
    _set_env(monkeypatch, {})
    name = "edges"
    c = pc.case(name)
    _, host_po, _ = run(name)
    pk = pc.packed(name)
    GUARD, JUNK = 256, 0x5A
    eng = Engine(c.params, memspace=capi.MA_MEM_DEVICE)
    arena = DeviceArena()
    try:
        bs = capi.make_batch_struct({k: arena.upload(v) for k, v in c.arrs.items()}, c.n, c.nr)

        def call(probe_arrays):
            # (the output arrays hold exactly the rows of THIS probe set: the call writes every probe's row)
            specs = [capi.asm_out_spec(c.params, c.n), capi.probe_out_spec(c.params, int(probe_arrays["probe_win_off"][c.n]))]
            ptrs =[{k: arena.upload_unaligned(np.zeros(int(sz), dt), shift=0, guard=GUARD, junk=JUNK) for k, (dt, sz) in spec.items()}
                    for spec in specs]
            pr_ptrs = {k: arena.upload(v) for k, v in probe_arrays.items()}
            rc = 0
            try:
                eng.assemble_probes_device(bs, capi.fill_struct(capi.AsmOut, ptrs[0]), capi.fill_struct(capi.Probes, pr_ptrs),
                                           capi.fill_struct(capi.ProbeOut, ptrs[1]))
            except EngineError as e:
                rc = e.rc
            eng.synchronize()
            for spec, pt in zip(specs, ptrs):
                for k, (dt, sz) in spec.items():
                    nbytes = int(sz) * np.dtype(dt).itemsize
                    front, behind = arena.download(pt[k] - GUARD, np.uint8, GUARD), arena.download(pt[k] + nbytes, np.uint8, GUARD)
                    assert (front == JUNK).all() and (behind == JUNK).all(), f"the guard of {k} changed"
            return rc, {k: arena.download(ptrs[1][k], dt, sz) for k, (dt, sz) in specs[1].items()}

        rc, dev_po = call(pk)
        assert rc == 0
        for k in host_po:
            assert dev_po[k].tobytes() == host_po[k].tobytes(), k
        # a probe that starts behind its window, one that ends behind it: MA_ERR_ARG from the kernel, their rows zero, every
        # other row as before
        L = int(c.arrs["ref_off"][1]) - int(c.arrs["ref_off"][0])
        bad = {k: v.copy() for k, v in pk.items()}
        bad["probe_pos"][0], bad["probe_pos"][2], bad["probe_ref_len"][2] = L + 5, L - 2, 3
        rc, bad_po = call(bad)
        assert rc == capi.MA_ERR_ARG
        got, ok = pc.engine_rows(name, bad_po), pc.engine_rows(name, dev_po)
        zero = {k: (0 if k in ("pb_k", "pb_alt_kmers") else [0] * len(v)) for k, v in ok[0][0].items()}
        assert got[0][0] == zero and got[0][2] == zero
        assert got[0][1] == ok[0][1] and got[0][3:] == ok[0][3:] and got[1:] == ok[1:]
        # more than 256 probes in a window, an ALT of more than 256 bases: MA_ERR_PARAM
        many = capi.pack_probes([[(7, 1, b"A")] * 257, [], [], []])
        assert call(many)[0] == capi.MA_ERR_PARAM
        long_alt = capi.pack_probes([[(7, 1, b"A" * 257)], [], [], []])
        assert call(long_alt)[0] == capi.MA_ERR_PARAM
    finally:
        eng.close()
        arena.close()


def test_a_capacity_retry_pass_takes_the_rows_with_it(monkeypatch):
    """The MA_ARENA_CAP=256 batch of tests/test_gpu_graph_export.py: the first pass reports windows with rows and
    MA_W_TABLE_OVERFLOW, the retry passes assemble them again from scratch -- their probe rows are cleared first and the call
    returns those of the pass that reported the window: the rows of a run with a roomy arena."""
    name = "retry"
    c = pc.case(name)
    _set_env(monkeypatch, {"MA_ARENA_CAP": "256", "MA_NO_CAP_RETRY": "1"})
    a1, _, _ = run(name)
    first = [w for w in range(c.n) if int(a1["win_status"][w]) & capi.MA_W_TABLE_OVERFLOW and int(a1["win_ncomp"][w]) > 0]
    assert first, "no window is reported with rows and a capacity flag: the test does not reach the retry's clearing"
    _set_env(monkeypatch, {"MA_ARENA_CAP": "256"})
    asm, po, _ = run(name)
    assert not (asm["win_status"] & capi.MA_W_TABLE_OVERFLOW).any()
    _set_env(monkeypatch, {})
    roomy_asm, roomy, _ = run(name)
    assert_same_assembly(c.params, roomy_asm, asm, c.n)
    for k in po:
        assert po[k].tobytes() == roomy[k].tobytes(), k
    rows = pc.engine_rows(name, po)
    assert all(any(any(r["pb_final"]) for r in rows[w]) for w in first), first


def test_arguments(monkeypatch):
    _set_env(monkeypatch, {})
    c = pc.case("gap")
    L = int(c.arrs["ref_off"][1])
    eng = Engine(c.params)

    def rc_of(per_window=None, drop=None, drop_out=None, drop_asm=None):
        pk = capi.pack_probes(per_window if per_window is not None else [[(7, 1, b"A")]])
        P = int(pk["probe_win_off"][c.n])
        asm = capi.alloc_host(capi.asm_out_spec(c.params, c.n))
        po = capi.alloc_host({k: (dt, max(sz, 1)) for k, (dt, sz) in capi.probe_out_spec(c.params, P).items()})
        for d, k in ((pk, drop), (po, drop_out), (asm, drop_asm)):
            if k:
                d.pop(k)
        try:
            eng.assemble_probes_device(capi.make_batch_struct(c.arrs, c.n, c.nr), capi.fill_struct(capi.AsmOut, asm),
                                       capi.fill_struct(capi.Probes, pk), capi.fill_struct(capi.ProbeOut, po))
        except EngineError as e:
            return e.rc
        return 0

    try:
        assert rc_of() == 0
        assert rc_of([[(L - 1, 1, b"A"), (L - 31, 31, b"A")]]) == 0                  # the last base; a REF that ends with the window
        assert rc_of([[(L, 1, b"A")]]) == capi.MA_ERR_ARG                            # starts behind the window
        assert rc_of([[(L - 1, 2, b"A")]]) == capi.MA_ERR_ARG                        # ends behind it
        assert rc_of([[(7, 1, b"A" * 256), (7, 256, b"A")]]) == 0                    # alleles at the limit
        assert rc_of([[(7, 1, b"A" * 257)]]) == capi.MA_ERR_PARAM
        assert rc_of([[(7, 257, b"A")]]) == capi.MA_ERR_PARAM
        assert rc_of([[(7, 1, b"A")] * 256]) == 0                                    # probes at the limit
        assert rc_of([[(7, 1, b"A")] * 257]) == capi.MA_ERR_PARAM
        for k in capi.PROBE_DTYPES:
            assert rc_of(drop=k) == capi.MA_ERR_ARG, k
        for k in capi.probe_out_spec(c.params, 1):
            assert rc_of(drop_out=k) == capi.MA_ERR_ARG, k
        for k in ("win_k", "win_ncomp", "comp_hap0", "comp_nhaps", "hap_len", "hap_bases"):
            assert rc_of(drop_asm=k) == capi.MA_ERR_ARG, k
        # probes or probe_out NULL: the plain call, none of the probe kernels
        asm = capi.alloc_host(capi.asm_out_spec(c.params, c.n))
        pk = capi.pack_probes([[(7, 1, b"A")]])
        eng.assemble_probes_device(capi.make_batch_struct(c.arrs, c.n, c.nr), capi.fill_struct(capi.AsmOut, asm), None, None)
        assert not {k for k, _ in eng.kernel_times()} & PROBE_KERNELS
        eng.assemble_probes_device(capi.make_batch_struct(c.arrs, c.n, c.nr), capi.fill_struct(capi.AsmOut, asm),
                                   capi.fill_struct(capi.Probes, pk), None)
        assert not {k for k, _ in eng.kernel_times()} & PROBE_KERNELS
        plain = eng.assemble(c.arrs, c.n, c.nr)
        assert_same_assembly(c.params, plain, asm, c.n)
    finally:
        eng.close()
    assert C.sizeof(capi.Probes) == 48 and C.sizeof(capi.ProbeOut) == 48
