// Stand-alone driver of opt_amd/csrc/graph_partition.h for tests/test_graph_partition_cpu.py (built with -fsanitize=address,undefined, run as a child process).
// stdin-free: argv[1] = case file "N nE V cap nRequests r_0 .. r_{n-1}" followed by V * nE indices (slot-major); for every requested workgroup count it prints the partition:
//   partition <requested> <G> <nWires> <evaluated> <heldMax> <haloMax> <edgesMax>
//   owner <N ints>
//   part <g> <nOwn> <nHeld> <nEdges> <nInc>  then one line each: held, edge, slot, incOff, incIdx, wire, haloWire
#include "graph_partition.h"

#include <cstdio>
#include <cstdlib>

static void line(const char* name, const std::vector<int>& v) {
    std::printf("%s", name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long N = 0; int nE = 0, V = 0, cap = 0, nReq = 0;
    if (std::fscanf(f, "%ld %d %d %d %d", &N, &nE, &V, &cap, &nReq) != 5) return 2;
    std::vector<int> req((size_t)nReq);
    for (int& r : req) if (std::fscanf(f, "%d", &r) != 1) return 2;
    std::vector<std::vector<int>> idx((size_t)V, std::vector<int>((size_t)nE));
    for (auto& col : idx) for (int& x : col) if (std::fscanf(f, "%d", &x) != 1) return 2;
    std::fclose(f);
    std::vector<const int*> ptr;
    for (auto& col : idx) ptr.push_back(col.data());
    for (int r : req) {
        const int G = optamd::graphPartitionClamp(N, r, cap);
        const optamd::GraphPartition P = optamd::buildGraphPartition(N, nE, V, ptr.data(), G);
        std::printf("partition %d %d %d %ld %d %d %d\n", r, P.G, P.nWires, P.evaluated, P.heldMax, P.haloMax, P.edgesMax);
        line("owner", P.owner);
        for (int g = 0; g < P.G; ++g) {
            const optamd::GraphPart& Q = P.parts[(size_t)g];
            std::printf("part %d %d %zu %zu %zu\n", g, Q.nOwn, Q.held.size(), Q.edge.size(), Q.incIdx.size());
            line("held", Q.held); line("edge", Q.edge); line("slot", Q.slot); line("incOff", Q.incOff); line("incIdx", Q.incIdx); line("wire", Q.wire); line("haloWire", Q.haloWire);
        }
    }
    return 0;
}
