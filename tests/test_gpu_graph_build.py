"""ma_assemble_graph_batch against tests/graph_build_ref.py: the graph the engine exports for every reported component must BE
the graph a plain restatement of the reference's build + prune makes from the batch's reads at the reported k -- node for node
(sequence, per-sample counts, sign, label, anchor flags) and edge for edge (source, destination, kind), exactly, on the cases of
tests/graph_build_cases.py and on the three clean routes.  tests/test_graph_build_ref.py shows without a GPU that the same
graphs explain the oracle's rows, that every case reaches its edge, and that this comparison reports a changed count, a flipped
label bit and a dropped edge."""
import pytest

import graph_build_cases as gc
import graph_build_ref as gb
import graph_export_ref as ref
from lancet2_amd.engine import Engine

pytestmark = pytest.mark.gpu

ROUTE_ENVS = {"compact": {}, "raw": {"MA_NO_CHAINS": "1"}, "large classes": {"MA_CHAINS_CAP": "64"}}
RUNS = [(name, route) for name, three in (("c2", True), ("c3_ladder", False), ("c5_three_samples", False), ("c4_deep", False),
                                          ("handmade", True)) for route in (ROUTE_ENVS if three else ("compact",))]  # gc.cases()' names


@pytest.mark.parametrize("name,route", RUNS)
def test_exported_graph_is_the_restatements(name, route, monkeypatch):
    for k in ("MA_NO_CHAINS", "MA_CHAINS_CAP", "MA_NO_SPEC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTE_ENVS[route].items():
        monkeypatch.setenv(k, v)
    c = gc.cases()[name]
    assert {n for n, _ in RUNS} == set(gc.cases()) and c.three_routes == ((name, "raw") in RUNS)
    S = c.params.num_samples
    eng = Engine(c.params)
    try:
        asm, gr = eng.assemble_graph(c.arrs, c.n, c.nr, *c.caps)
    finally:
        eng.close()
    compared, complaints = [], []
    for w in range(c.n):
        if not gc.comparable(asm, w):
            continue
        assert int(gr["win_gstatus"][w]) == 0, (w, int(gr["win_nnodes"][w]), int(gr["win_nedges"][w]), int(gr["win_nseq"][w]))
        want = ref.graph_key(gc.expected_arrays(name, w, asm), 0, S)  # (asserts that every comp_* row finds its component)
        got = ref.graph_key(gr, w, S)
        diff = gb.first_difference(got, want)
        print(f"{name} [{route}] w{w} k={int(asm['win_k'][w])}: {sum(len(v[0]) for v in got.values())} nodes, "
              f"{sum(len(v[1]) for v in got.values())} edges: {'equal' if diff is None else diff}")
        if diff is not None:
            complaints.append(f"w{w} k={int(asm['win_k'][w])} (engine | restatement): {diff}")
        compared.append(w)
    assert not complaints, "\n".join(complaints[:10])
    assert len(compared) >= c.min_compared and 2 * len(compared) >= c.n, compared
    if c.handmade:
        assert compared == list(range(c.n))
