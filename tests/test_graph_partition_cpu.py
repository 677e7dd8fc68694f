"""CPU test (no GPU): the host-side partition of a hypergraph over the workgroups of one persistent launch (opt_amd/csrc/graph_partition.h; solver parameter
amd_onchip = 7, graph_onchip_grid.h).  The header is plain C++: it is compiled here into a stand-alone driver (tests/graph_partition_driver.cpp, its own main) with the
address and undefined-behaviour sanitizers and run as a child process on the graphs of tests/graph_cases.py, for 1, 2, 3, 8 and 32 workgroups and for more workgroups than
vertices.  What is asserted is what ge_onchipPcgGrid relies on:

  every vertex has one owner and no part is empty after clamping;
  a hyperedge is evaluated by exactly the workgroups that own one of its vertices, and its |J p|^2 is counted by exactly one of them (the owner of its slot-0 vertex);
  every slot of every evaluated hyperedge maps to a held local index, and the map inverts;
  the incidence list of every owned vertex is complete and ascending in the global id slot * nE + hyperedge;
  every vertex that is halo somewhere has a wire, its owner sends on it and every holder receives on it;
  parts follow connectivity: the shuffled raptor evaluates within 5 % of the hyperedges the ordered raptor does at the same workgroup count.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import graph_cases as gc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "opt_amd", "csrc")
CAP = 32
REQUESTS = (1, 2, 3, 8, 32, 100000)      # the last: more than any case has vertices


def _cases():
    arm = lambda e: gc.base_problem(e, "armadillo", False)
    return {
        "open_patch_cotangent": lambda: gc.base_problem("cotangent", "open_patch", False),      # 35 vertices; four hyperedges with v2 == v3
        "open_patch_embedded": lambda: gc.base_problem("embedded", "open_patch", False),
        "armadillo_cotangent": lambda: arm("cotangent"),
        "armadillo_embedded": lambda: arm("embedded"),
        "raptor_embedded": lambda: gc.base_problem("embedded", "raptor", False),
        "raptor_embedded_shuffled": lambda: gc.reorder(gc.base_problem("embedded", "raptor", False), "shuffle", seed=3),
        "raptor_cotangent": lambda: gc.base_problem("cotangent", "raptor", False),
        "raptor_cotangent_shuffled": lambda: gc.reorder(gc.base_problem("cotangent", "raptor", False), "shuffle", seed=3),
        "hub_embedded": lambda: gc.with_hub(arm("embedded"), 64),
        "hub_cotangent": lambda: gc.with_hub(arm("cotangent"), 64),
        "isolated_vertex": lambda: gc.with_isolated_vertex(arm("robust")),
        "tail_only_vertex": lambda: gc.with_tail_only_vertex(arm("cotangent")),
        "duplicate_hyperedges": lambda: gc.with_duplicate_edges(arm("cotangent"), 9),
    }


CASES = _cases()


def _tiny_cases():
    """Graphs with fewer vertices than the cap of 32: a request of N or more gives every workgroup exactly one vertex (the clamp to one vertex per workgroup)."""
    path = np.arange(4)
    quad = np.array([[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [5, 0, 1, 1]]).T      # (the last hyperedge repeats a vertex)
    return {"tiny_path": (5, [np.r_[path, path + 1], np.r_[path + 1, path]]), "tiny_hyperedges": (7, [c for c in quad]), "tiny_single_vertex": (1, [np.array([0]), np.array([0])])}


TINY = _tiny_cases()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the driver"
    exe = str(tmp_path_factory.mktemp("partition") / "graph_partition_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                           os.path.join(HERE, "graph_partition_driver.cpp"), "-o", exe])
    return exe


def _ints(line, name):
    t = line.split()
    assert t[0] == name, (t[0], name)
    return np.array(t[1:], dtype=np.int64)


def _run(driver, P, tmp):
    if isinstance(P, tuple):
        N, idx = P
    else:
        N, idx = gc.n_vertices(P), gc.index_arrays(P)
    nE, V = len(idx[0]), len(idx)
    path = os.path.join(tmp, "case.txt")
    with open(path, "w") as f:
        f.write(f"{N} {nE} {V} {CAP} {len(REQUESTS)} " + " ".join(map(str, REQUESTS)) + "\n")
        for c in idx:
            f.write(" ".join(map(str, c.tolist())) + "\n")
    r = subprocess.run([driver, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    out, i = {}, 0
    while i < len(lines):
        t = lines[i].split()
        assert t[0] == "partition"
        req, G = int(t[1]), int(t[2])
        rec = dict(G=G, nWires=int(t[3]), evaluated=int(t[4]), heldMax=int(t[5]), haloMax=int(t[6]), edgesMax=int(t[7]), owner=_ints(lines[i + 1], "owner"), parts=[])
        i += 2
        for g in range(G):
            h = lines[i].split()
            assert h[0] == "part" and int(h[1]) == g
            part = dict(nOwn=int(h[2]))
            for k, name in enumerate(("held", "edge", "slot", "incOff", "incIdx", "wire", "haloWire")):
                part[name] = _ints(lines[i + 1 + k], name)
            assert len(part["held"]) == int(h[3]) and len(part["edge"]) == int(h[4]) and len(part["incIdx"]) == int(h[5])
            rec["parts"].append(part)
            i += 8
        out[req] = rec
    return (N, nE, V, np.stack(idx).astype(np.int64)), out


@pytest.fixture(scope="module")
def results(driver, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("partition_cases"))
    out = {name: _run(driver, make(), tmp) for name, make in CASES.items()}
    out.update({name: _run(driver, case, tmp) for name, case in TINY.items()})
    return out


def _check(N, nE, V, idx, req, R):
    G = R["G"]
    assert G == max(1, min(req, CAP, N))
    owner = R["owner"]
    assert len(owner) == N and owner.min() >= 0 and owner.max() < G
    assert np.all(np.bincount(owner, minlength=G) >= 1), "an empty part"      # every vertex owned once (one entry each), no part empty
    edge_owners = [set(owner[idx[:, e]].tolist()) for e in range(nE)]
    flat = idx.reshape(-1)      # position slot * nE + e
    by_vertex = np.argsort(flat, kind="stable")
    first = np.searchsorted(flat[by_vertex], np.arange(N + 1))      # ids of vertex v, ascending: by_vertex[first[v]:first[v + 1]]
    evaluated_by = [set() for _ in range(nE)]
    counted = np.zeros(nE, dtype=np.int64)
    senders, receivers = {}, {}
    for g, Q in enumerate(R["parts"]):
        held, nOwn, edge = Q["held"], Q["nOwn"], Q["edge"]
        ne = len(edge)
        assert sorted(held[:nOwn].tolist()) == np.flatnonzero(owner == g).tolist()
        assert len(set(held.tolist())) == len(held) and np.all(owner[held[nOwn:]] != g)
        assert np.all(np.diff(edge) > 0)      # ascending: local record ids ascend exactly when global ids do
        slot = Q["slot"].reshape(V, ne) if ne else np.zeros((V, 0), dtype=np.int64)
        assert slot.size == 0 or (slot.min() >= 0 and slot.max() < len(held))
        assert np.array_equal(held[slot], idx[:, edge]), "a slot does not map back to its vertex"      # the map inverts
        assert set(np.unique(slot).tolist()) | set(range(nOwn)) == set(range(len(held))), "a halo vertex no evaluated hyperedge names"
        for le, e in enumerate(edge):
            evaluated_by[e].add(g)
            counted[e] += int(slot[0, le] < nOwn)
        # incidence: per owned vertex the local record ids, complete and ascending in the global id
        off, inc = Q["incOff"], Q["incIdx"]
        assert len(off) == nOwn + 1 and off[0] == 0 and off[-1] == len(inc)
        for i in range(nOwn):
            ids = inc[off[i]:off[i + 1]]
            j, le = ids // max(ne, 1), ids % max(ne, 1)
            glob = j * nE + edge[le]
            assert np.all(np.diff(glob) > 0)
            want = by_vertex[first[held[i]]:first[held[i] + 1]]      # ids slot * nE + e of the whole graph
            assert np.array_equal(glob, want), (g, i)
        assert len(Q["wire"]) == nOwn and len(Q["haloWire"]) == len(held) - nOwn
        for i in range(nOwn):
            if Q["wire"][i] >= 0:
                assert held[i] not in senders
                senders[int(held[i])] = int(Q["wire"][i])
        for h, v in enumerate(held[nOwn:]):
            receivers.setdefault(int(v), []).append((g, int(Q["haloWire"][h])))
    for e in range(nE):
        assert evaluated_by[e] == edge_owners[e], e
    assert np.all(counted == 1), "|J p|^2 of a hyperedge counted other than once"
    assert R["evaluated"] == sum(len(s) for s in edge_owners)
    # wires: a vertex is halo elsewhere iff some hyperedge joins it to a vertex of another owner
    halo_elsewhere = {int(v) for e in range(nE) if len(edge_owners[e]) > 1 for v in idx[:, e]}
    assert set(senders) == halo_elsewhere and set(receivers) == halo_elsewhere
    assert sorted(senders.values()) == list(range(R["nWires"]))
    holders = {}      # vertex -> the workgroups that evaluate one of its hyperedges
    for e in range(nE):
        for v in idx[:, e]:
            holders.setdefault(int(v), set()).update(edge_owners[e])
    for v, rs in receivers.items():
        assert all(w == senders[v] for _, w in rs)
        assert {g for g, _ in rs} == holders[v] - {int(owner[v])}, v
    assert R["heldMax"] == max(len(Q["held"]) for Q in R["parts"]) and R["edgesMax"] == max(len(Q["edge"]) for Q in R["parts"])


@pytest.mark.parametrize("req", REQUESTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_partition_invariants(results, name, req):
    (N, nE, V, idx), out = results[name]
    _check(N, nE, V, idx, req, out[req])


@pytest.mark.parametrize("req", REQUESTS)
@pytest.mark.parametrize("name", sorted(TINY))
def test_fewer_vertices_than_the_cap(results, name, req):
    (N, nE, V, idx), out = results[name]
    assert N < CAP
    _check(N, nE, V, idx, req, out[req])
    if req >= N:
        assert out[req]["G"] == N and all(Q["nOwn"] == 1 for Q in out[req]["parts"])


def test_one_workgroup_holds_the_whole_graph(results):
    (N, nE, V, idx), out = results["armadillo_cotangent"]
    R = out[1]
    assert R["G"] == 1 and R["nWires"] == 0 and R["evaluated"] == nE and R["heldMax"] == N


@pytest.mark.parametrize("energy", ["embedded", "cotangent"])
@pytest.mark.parametrize("req", [2, 3, 8, 32])
def test_parts_follow_connectivity_not_hyperedge_order(results, energy, req):
    """The shuffled raptor evaluates within 5 % of the hyperedges of the ordered raptor at the same workgroup count."""
    a = results[f"raptor_{energy}"][1][req]["evaluated"]
    b = results[f"raptor_{energy}_shuffled"][1][req]["evaluated"]
    assert abs(a - b) <= 0.05 * a, (a, b)
