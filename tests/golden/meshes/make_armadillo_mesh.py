#!/usr/bin/env python
"""Freeze the input of the reference's arap_mesh_deformation example as a fixture: examples/data/small_armadillo.ply (130 vertices, 256 triangles), its landmark file
small_armadillo.mrk, and the mesh after ONE sqrt(3) subdivision step (386 vertices: what the example solves on, arap_mesh_deformation/src/main.cpp:58-79)
-> tests/golden/meshes/armadillo_mesh.npz (a directory of its own: tests/test_golden.py reads every tests/golden/*.npz as a frozen oracle run).  The landmark file indexes the SUBDIVIDED mesh (the example attaches the markers after subdividing); marker_index_coarse is the same
handle on the 130-vertex mesh: the vertex itself if it is an old one, else the first corner of the face whose centroid the marker sits on.

Data only (vertex positions, triangle indices, marker indices / targets), read with opt_amd.io.read_ply / read_mrk.  The subdivision is plain numpy, Kobbelt's sqrt(3)
rule as the example's subdivider applies it: one new vertex per face at its centroid; every interior old edge is replaced by the edge between the centroids of its two
faces (an edge flip), a boundary edge stays; an old interior vertex of valence n moves to (1 - a) v + a * mean(old one-ring), a = (4 - 2 cos(2 pi / n)) / 9 (a boundary
vertex stays).  The smoothing matters to the tests: with the old vertices left in place every new vertex lies in the plane of its three old neighbours, and on that mesh
the third Gauss-Newton step of a 3 x 25 solve amplifies a last-bit difference of the PCG sums 5e5 times -- the CPU oracle under the reference's own summation order
(set_reduction(1, seed), seeds 1-5) is 1e-11 .. 5e-11 from its exact-order run there, and 2e-16 .. 2e-15 on the smoothed mesh.  Run where the reference's data
directory is at hand:
    python tests/golden/meshes/make_armadillo_mesh.py <data directory>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
from opt_amd import io      # noqa: E402


def sqrt3_subdivide(V, F):
    V = np.asarray(V, dtype=np.float64)
    F = [tuple(f) for f in F]
    centroid = len(V) + np.arange(len(F))
    Vn = np.concatenate([V, np.array([V[list(f)].mean(0) for f in F])])
    ring = [set() for _ in V]
    edge_faces = {}
    for f in F:
        for a, b in zip(f, f[1:] + f[:1]):
            ring[a].add(b); ring[b].add(a)
            edge_faces[(min(a, b), max(a, b))] = edge_faces.get((min(a, b), max(a, b)), 0) + 1
    boundary = {v for e, c in edge_faces.items() if c == 1 for v in e}
    for v, nb in enumerate(ring):      # the old vertices, smoothed from the OLD positions of their one-ring
        if nb and v not in boundary:
            a = (4.0 - 2.0 * np.cos(2.0 * np.pi / len(nb))) / 9.0
            Vn[v] = (1.0 - a) * V[v] + a * V[sorted(nb)].mean(0)
    faces_of = {}
    for fi, f in enumerate(F):
        for a, b in zip(f, f[1:] + f[:1]):
            faces_of.setdefault((min(a, b), max(a, b)), []).append((fi, a, b))
    Fn = []
    for (lo, hi), fs in sorted(faces_of.items()):
        if len(fs) == 2:        # interior edge (a, b) of faces f, g: triangles (a, c_g, c_f) and (b, c_f, c_g), oriented like f
            (f, a, b), (g, _, _) = fs
            Fn.append((a, int(centroid[g]), int(centroid[f])))
            Fn.append((b, int(centroid[f]), int(centroid[g])))
        else:                   # boundary edge: it stays, with the centroid of its one face
            f, a, b = fs[0]
            Fn.append((a, b, int(centroid[f])))
    return Vn, Fn


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_armadillo_mesh.py <the reference's examples/data directory>")
    data = sys.argv[1]
    V, F = io.read_ply(os.path.join(data, "small_armadillo.ply"))
    idx, pos = io.read_mrk(os.path.join(data, "small_armadillo.mrk"))
    V2, F2 = sqrt3_subdivide(V, F)
    coarse = np.array([i if i < len(V) else F[i - len(V)][0] for i in idx], dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "armadillo_mesh.npz"), vertices=V.astype(np.float32), faces=np.array(F, dtype=np.int32),
                        marker_index=idx.astype(np.int32), marker_index_coarse=coarse, marker_position=pos.astype(np.float32),
                        vertices_sub=V2.astype(np.float32), faces_sub=np.array(F2, dtype=np.int32))
    for name, (vv, ff) in {"small_armadillo": (V, F), "subdivided": (V2, F2)}.items():
        h, _ = io.mesh_half_edges(len(vv), [list(f) for f in ff])
        print(name, len(vv), "vertices,", len(ff), "faces, valence", np.bincount(h).min(), "-", np.bincount(h).max(), ",", len(idx), "markers")
