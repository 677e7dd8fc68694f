#!/usr/bin/env python
"""Freeze the input of the reference's cotangent_mesh_smoothing example as a fixture: examples/data/head.ply (689 vertices, 1355 triangles; 4086 cotangent hyperedges,
one per (vertex, ring neighbour)) -> tests/golden/meshes/head_mesh.npz.  It is the mesh the one-workgroup solve of the functor mesh energies (solver parameter
amd_onchip = 6, opt_amd/csrc/graph_onchip.h) serves with two vertices per lane: tests/test_onchip_graph_gpu.py, tools/bench_onchip_graph.py.

Data only (vertex positions, triangle indices), read with opt_amd.io.read_ply.  Run where the reference's data directory is at hand:
    python tests/golden/meshes/make_head_mesh.py <data directory>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
from opt_amd import io      # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_head_mesh.py <the reference's examples/data directory>")
    V, F = io.read_ply(os.path.join(sys.argv[1], "head.ply"))
    np.savez_compressed(os.path.join(HERE, "head_mesh.npz"), vertices=np.asarray(V, dtype=np.float32), faces=np.array(F, dtype=np.int32))
    h, _ = io.mesh_half_edges(len(V), [list(f) for f in F])
    print("head", len(V), "vertices,", len(F), "faces,", len(h), "half-edges, valence", np.bincount(h).min(), "-", np.bincount(h).max())
