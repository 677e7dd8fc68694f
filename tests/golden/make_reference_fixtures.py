#!/usr/bin/env python
"""Record what the CPU tests need from the reference checkout, so that they run without it.

    python tests/golden/make_reference_fixtures.py --reference DIR        (DIR = a checkout of the reference project; needs g++)

Writes, under tests/golden/:
  reference_data/cat512.constraints, reference_data/shape_from_shading/default.SFSSolverParameters
                                      the reference's example inputs as they are (tests/test_io.py)
  reference_data/shape_from_shading/default_*.imagedump.xz
                                      the SFS example's 640x480 imagedumps, xz-compressed byte for byte (tests/test_io.py decompresses them)
  reference_data/comparator_iw_23x17.npz
                                      what the reference's hand-written image_warping comparator maths (examples/image_warping/src/WarpingSolverEquations.h)
                                      computes on tests/test_reference_comparator_cpu.py's input: F, -J^T F and J^T J v per variable
Only data is stored: the reference's example inputs and the comparator's recorded outputs.
"""
import argparse
import glob
import lzma
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)

# The comparator header is compiled where it lies, against this stand-in for <cuda_runtime.h> (vector types and empty qualifiers).
STANDIN = r'''
#pragma once
#include <cmath>
#include <cstring>
#include <limits>
#define __device__
#define __host__
#define __inline__ inline
#define __forceinline__ inline
#define __shared__
#define __global__
struct float2 { float x, y; float2() {} float2(float a, float b) : x(a), y(b) {} };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; }; struct int3 { int x, y, z; }; struct int4 { int x, y, z, w; };
struct uint2 { unsigned x, y; }; struct uint3 { unsigned x, y, z; }; struct uint4 { unsigned x, y, z, w; };
struct uchar4 { unsigned char x, y, z, w; };
inline float2 make_float2(float x, float y) { return float2(x, y); }
inline float3 make_float3(float x, float y, float z) { float3 r; r.x = x; r.y = y; r.z = z; return r; }
inline float4 make_float4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
inline int2 make_int2(int x, int y) { int2 r; r.x = x; r.y = y; return r; }
inline int3 make_int3(int x, int y, int z) { int3 r; r.x = x; r.y = y; r.z = z; return r; }
inline int4 make_int4(int x, int y, int z, int w) { int4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
inline uint2 make_uint2(unsigned x, unsigned y) { uint2 r; r.x = x; r.y = y; return r; }
inline uint3 make_uint3(unsigned x, unsigned y, unsigned z) { uint3 r; r.x = x; r.y = y; r.z = z; return r; }
inline uchar4 make_uchar4(unsigned char x, unsigned char y, unsigned char z, unsigned char w) { uchar4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
typedef int cudaError; typedef int cudaError_t;
enum { cudaSuccess = 0, cudaMemcpyDeviceToHost = 2, cudaMemcpyHostToDevice = 1 };
inline const char* cudaGetErrorString(int) { return "stand-in"; }
inline int cudaMemcpy(void* d, const void* s, size_t n, int) { memcpy(d, s, n); return 0; }
inline void __syncthreads() {}
inline float __shfl_down(float v, int, int) { return v; }
inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
'''

DRIVER = r'''
#include "%(hdr)s/WarpingSolverState.h"
#include "%(hdr)s/WarpingSolverParameters.h"
#include "%(hdr)s/WarpingSolverEquations.h"
#include <cstdio>
#include <vector>
float bucket[2048];
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    int W, H; float wf, wr;
    fread(&W, 4, 1, f); fread(&H, 4, 1, f); fread(&wf, 4, 1, f); fread(&wr, 4, 1, f);
    const int N = W * H;
    std::vector<float2> x(N), ur(N), con(N), p(N), delta(N), pre(N); std::vector<float> A(N), mask(N), pA(N), deltaA(N), preA(N);
    fread(x.data(), 8, N, f); fread(A.data(), 4, N, f); fread(ur.data(), 8, N, f); fread(con.data(), 8, N, f); fread(mask.data(), 4, N, f);
    fread(p.data(), 8, N, f); fread(pA.data(), 4, N, f); fclose(f);
    SolverInput in; in.N = N; in.width = W; in.height = H; in.d_constraints = con.data();
    SolverState st; memset(&st, 0, sizeof st);
    st.d_x = x.data(); st.d_A = A.data(); st.d_urshape = ur.data(); st.d_mask = mask.data(); st.d_p = p.data(); st.d_pA = pA.data();
    st.d_delta = delta.data(); st.d_deltaA = deltaA.data(); st.d_precondioner = pre.data(); st.d_precondionerA = preA.data();
    SolverParameters pr; pr.weightFitting = wf; pr.weightRegularizer = wr; pr.nNonLinearIterations = 1; pr.nLinIterations = 1;
    FILE* o = fopen(argv[2], "wb");
    double F = 0;
    for (int i = 0; i < N; ++i) F += (double)evalFDevice(i, in, st, pr);
    fwrite(&F, 8, 1, o);
    for (int i = 0; i < N; ++i) { float bA; float2 b = evalMinusJTFDevice(i, in, st, pr, bA); float v[3] = {b.x, b.y, bA}; fwrite(v, 4, 3, o); }
    for (int i = 0; i < N; ++i) { float bA; float2 b = applyJTJDevice(i, in, st, pr, bA); float v[3] = {b.x, b.y, bA}; fwrite(v, 4, 3, o); }
    fclose(o);
    return 0;
}
'''


def reference_data(ref):
    out = os.path.join(HERE, "reference_data")
    os.makedirs(os.path.join(out, "shape_from_shading"), exist_ok=True)
    data = os.path.join(ref, "examples", "data")
    shutil.copyfile(os.path.join(data, "cat512.constraints"), os.path.join(out, "cat512.constraints"))
    shutil.copyfile(os.path.join(data, "shape_from_shading", "default.SFSSolverParameters"), os.path.join(out, "shape_from_shading", "default.SFSSolverParameters"))
    for f in sorted(glob.glob(os.path.join(data, "shape_from_shading", "default_*.imagedump"))):
        with open(f, "rb") as src, open(os.path.join(out, "shape_from_shading", os.path.basename(f) + ".xz"), "wb") as dst:
            dst.write(lzma.compress(src.read(), preset=9 | lzma.PRESET_EXTREME))


def comparator(ref):
    from opt_amd import workloads as wl
    hdr = os.path.join(ref, "examples", "image_warping", "src")
    W, H = 23, 17
    P = wl.image_warping(W, H, random_state=19, mask_fraction=0.0, perturb=0.4)          # Mask == 0: the exact 2x relations hold
    v = np.random.default_rng(4).standard_normal(3 * W * H).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "cuda_runtime.h"), "w").write(STANDIN)
        open(os.path.join(tmp, "drv.cpp"), "w").write(DRIVER % {"hdr": hdr})
        exe = os.path.join(tmp, "drv")
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-w", "-fpermissive", f"-I{tmp}", f"-I{hdr}", os.path.join(tmp, "drv.cpp"), "-o", exe])
        blob = os.path.join(tmp, "in.bin")
        with open(blob, "wb") as f:
            f.write(np.array([W, H], dtype=np.int32).tobytes())
            f.write(np.array([float(P.params[5]) ** 2, float(P.params[6]) ** 2], dtype=np.float32).tobytes())   # weightFitting = w_fitSqrt^2 (CombinedSolver.h:126-130)
            for a in (P.params[0], P.params[1], P.params[2], P.params[3], P.params[4]):
                f.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
            f.write(v[:2 * W * H].tobytes()); f.write(v[2 * W * H:].tobytes())
        out = os.path.join(tmp, "out.bin")
        subprocess.check_call([exe, blob, out])
        raw = open(out, "rb").read()
    F = np.frombuffer(raw[:8], dtype=np.float64)[0]
    rest = np.frombuffer(raw[8:], dtype=np.float32).reshape(2, W * H, 3)
    np.savez(os.path.join(HERE, "reference_data", "comparator_iw_23x17.npz"), W=W, H=H, v=v, F=np.float64(F), minus_jtf=rest[0], jtj_v=rest[1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    a = ap.parse_args()
    reference_data(a.reference)
    comparator(a.reference)
