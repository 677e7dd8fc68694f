// Partition of a hypergraph's vertices over the workgroups of ONE persistent launch (graph_onchip_grid.h ge_onchipPcgGrid; solver parameter amd_onchip = 7).
// Plain C++, no HIP: tests/test_graph_partition_cpu.py compiles it into a stand-alone driver with the address and undefined-behaviour sanitizers.
//
//   every vertex has ONE owner workgroup;
//   a workgroup evaluates every hyperedge with at least one vertex it owns (a cut hyperedge is evaluated by every owner of one of its vertices: records never cross
//   workgroups) and holds every vertex of those hyperedges: its owned vertices first, then its halo;
//   |J p|^2 of a hyperedge is counted by the owner of its slot-0 vertex;
//   an owned vertex that is halo elsewhere gets a wire: the index under which its owner posts A p and its holders read it.
// Parts follow connectivity, not vertex index: recursive bisection of a breadth-first order started at a pseudo-peripheral vertex (the last vertex of a first sweep), so a
// shuffled mesh partitions like an ordered one and a part is a compact patch, not a ring of a sweep's level sets.
// All lists of a part carry LOCAL indices: vertices as positions in `held`, hyperedges as positions in `edge` (ascending global id), records as slot * nLocalEdges + position,
// which is ascending exactly when the global id slot * nE + e is.
#pragma once
#include <algorithm>
#include <numeric>
#include <vector>

namespace optamd {

struct GraphPart {
    int nOwn = 0;
    std::vector<int> held;        // global vertex ids: [0, nOwn) owned (ascending), then the halo (ascending)
    std::vector<int> edge;        // global hyperedge ids this part evaluates, ascending
    std::vector<int> slot;        // [V][edge.size()]: local vertex index of every slot
    std::vector<int> incOff;      // [nOwn + 1]
    std::vector<int> incIdx;      // local record ids of each owned vertex, ascending
    std::vector<int> wire;        // [nOwn]: the vertex's wire, or -1 (nobody else holds it)
    std::vector<int> haloWire;    // [held.size() - nOwn]: the wire its owner posts on
};
struct GraphPartition {
    int G = 0, V = 0, nE = 0, nWires = 0, heldMax = 0, haloMax = 0, edgesMax = 0;
    long N = 0, evaluated = 0;    // evaluated: hyperedge evaluations over all parts (>= nE)
    std::vector<int> owner;       // [N]
    std::vector<GraphPart> parts;
};

// the workgroup count a request becomes: at least one vertex per workgroup, at most `cap`
inline int graphPartitionClamp(long N, int requested, int cap) { return (int)std::max<long>(1, std::min<long>(std::min<long>(requested, cap), N)); }

// vidx[j][e]: vertex in slot j of hyperedge e.  G >= 1; clamp it with graphPartitionClamp first (G <= N: no part is empty).
inline GraphPartition buildGraphPartition(long N, int nE, int V, const int* const* vidx, int G) {
    GraphPartition P;
    P.G = G; P.V = V; P.nE = nE; P.N = N;
    const int n = (int)N;
    // vertex -> hyperedges (CSR), for the sweeps
    std::vector<int> off((size_t)n + 1, 0), adj((size_t)nE * V);
    for (int j = 0; j < V; ++j) for (int e = 0; e < nE; ++e) ++off[(size_t)vidx[j][e] + 1];
    for (int v = 0; v < n; ++v) off[(size_t)v + 1] += off[v];
    { std::vector<int> cur(off.begin(), off.end() - 1); for (int e = 0; e < nE; ++e) for (int j = 0; j < V; ++j) adj[(size_t)cur[vidx[j][e]]++] = e; }

    // breadth-first order of the vertices of `set` (mark[v] == id), every component in turn; `from`: where the first sweep starts
    std::vector<int> mark((size_t)n, 0), seen((size_t)n, -1);
    int sweep = 0;
    auto bfs = [&](const std::vector<int>& set, int id, int from, std::vector<int>& order) {
        order.clear(); ++sweep;
        auto run = [&](int s) {
            size_t head = order.size();
            seen[s] = sweep; order.push_back(s);
            for (; head < order.size(); ++head) {
                const int v = order[head];
                for (int t = off[v]; t < off[(size_t)v + 1]; ++t)
                    for (int j = 0; j < V; ++j) { const int w = vidx[j][adj[t]]; if (mark[w] == id && seen[w] != sweep) { seen[w] = sweep; order.push_back(w); } }
            }
        };
        run(from);
        for (int v : set) if (seen[v] != sweep) run(v);
    };
    P.owner.assign((size_t)n, 0);
    int nextId = 1;
    // split `set` (all marked `id`) over workgroups [g0, g0 + g)
    struct Job { std::vector<int> set; int id, g0, g; };
    std::vector<Job> jobs;
    { Job all; all.set.resize((size_t)n); std::iota(all.set.begin(), all.set.end(), 0); all.id = 0; all.g0 = 0; all.g = G; jobs.push_back(std::move(all)); }
    std::vector<int> order, order2;
    while (!jobs.empty()) {
        Job job = std::move(jobs.back()); jobs.pop_back();
        if (job.g == 1) { for (int v : job.set) P.owner[v] = job.g0; continue; }
        bfs(job.set, job.id, job.set[0], order);
        bfs(job.set, job.id, order.back(), order2);      // from the far end of the first sweep
        const int gl = job.g / 2, gr = job.g - gl;
        const size_t nl = job.set.size() * (size_t)gl / (size_t)job.g;      // >= gl whenever set.size() >= g
        Job L, R;
        L.set.assign(order2.begin(), order2.begin() + (long)nl); R.set.assign(order2.begin() + (long)nl, order2.end());
        L.id = nextId++; R.id = nextId++; L.g0 = job.g0; L.g = gl; R.g0 = job.g0 + gl; R.g = gr;
        for (int v : L.set) mark[v] = L.id;
        for (int v : R.set) mark[v] = R.id;
        jobs.push_back(std::move(R)); jobs.push_back(std::move(L));
    }

    // wires: an owned vertex some other part holds
    std::vector<int> wireOf((size_t)n, -1);
    for (int e = 0; e < nE; ++e)
        for (int j = 0; j < V; ++j)
            for (int i = 0; i < V; ++i)
                if (P.owner[vidx[j][e]] != P.owner[vidx[i][e]]) wireOf[vidx[j][e]] = 0;
    for (int v = 0; v < n; ++v) if (wireOf[v] == 0) wireOf[v] = P.nWires++;

    P.parts.resize((size_t)G);
    std::vector<int> local((size_t)n, -1), stamp((size_t)nE, -1);
    for (int g = 0; g < G; ++g) {
        GraphPart& Q = P.parts[(size_t)g];
        for (int v = 0; v < n; ++v) if (P.owner[v] == g) Q.held.push_back(v);
        Q.nOwn = (int)Q.held.size();
        for (int i = 0; i < Q.nOwn; ++i)
            for (int t = off[Q.held[i]]; t < off[(size_t)Q.held[i] + 1]; ++t) if (stamp[adj[t]] != g) { stamp[adj[t]] = g; Q.edge.push_back(adj[t]); }
        std::sort(Q.edge.begin(), Q.edge.end());
        std::vector<int> halo;
        for (int i = 0; i < Q.nOwn; ++i) local[Q.held[i]] = i;
        for (int e : Q.edge) for (int j = 0; j < V; ++j) { const int v = vidx[j][e]; if (P.owner[v] != g && local[v] < 0) { local[v] = 0; halo.push_back(v); } }
        std::sort(halo.begin(), halo.end());
        for (int v : halo) { local[v] = (int)Q.held.size(); Q.held.push_back(v); Q.haloWire.push_back(wireOf[v]); }
        const int ne = (int)Q.edge.size();
        Q.slot.resize((size_t)V * ne);
        Q.incOff.assign((size_t)Q.nOwn + 1, 0);
        for (int j = 0; j < V; ++j) for (int le = 0; le < ne; ++le) {
            const int l = local[vidx[j][Q.edge[le]]];
            Q.slot[(size_t)j * ne + le] = l;
            if (l < Q.nOwn) ++Q.incOff[(size_t)l + 1];
        }
        for (int i = 0; i < Q.nOwn; ++i) Q.incOff[(size_t)i + 1] += Q.incOff[i];
        Q.incIdx.resize((size_t)Q.incOff[Q.nOwn]);
        { std::vector<int> cur(Q.incOff.begin(), Q.incOff.end() - 1);      // (slot-major, position-minor: ascending record ids per vertex)
          for (int j = 0; j < V; ++j) for (int le = 0; le < ne; ++le) { const int l = Q.slot[(size_t)j * ne + le]; if (l < Q.nOwn) Q.incIdx[(size_t)cur[l]++] = j * ne + le; } }
        Q.wire.resize((size_t)Q.nOwn);
        for (int i = 0; i < Q.nOwn; ++i) Q.wire[i] = wireOf[Q.held[i]];
        for (int v : Q.held) local[v] = -1;
        P.evaluated += ne;
        P.heldMax = std::max(P.heldMax, (int)Q.held.size());
        P.haloMax = std::max(P.haloMax, (int)Q.held.size() - Q.nOwn);
        P.edgesMax = std::max(P.edgesMax, ne);
    }
    return P;
}

}  // namespace optamd
