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
  reference_data/comparator_<case>.npz
                                      the same for the poisson, ARAP and SFS comparator headers on the problems of tests/reference_cases.py:
                                      F, b = evalMinusJTFDevice, applyJTJDevice(v), the preconditioner (poisson, ARAP) or the diagonal read off
                                      25 period-5 probes of applyJTJDevice (SFS, after checking that its stencil reaches 2 pixels), and the
                                      iterates x_1..x_3 of a PCG run on that operator preconditioned as Opt does.  Each header is compiled as
                                      written (float) and widened to double; the widened outputs are stored, and only if they match the float
                                      build to float rounding.  The SFS precompute (Precompute_Kernel lives in a .cu file) is done by the driver
                                      with the header's own calShading2depthGradCompute.
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


# The poisson, ARAP and SFS drivers compile their header twice: as written (REF_REAL float) and widened (REF_REAL double: the driver
# defines `float` as `double` and sends the float-only math calls to the double ones before including the header).  This stand-in
# carries the vector types in REF_REAL; it is included before that define, so its own `float` stays float.
STANDIN_REAL = r"""
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
typedef REF_REAL ref_real;
struct float2 { ref_real x, y; float2() {} float2(ref_real a, ref_real b) : x(a), y(b) {} };
struct float3 { ref_real x, y, z; };
struct float4 { ref_real x, y, z, w; };
struct int2 { int x, y; }; struct int3 { int x, y, z; }; struct int4 { int x, y, z, w; };
struct uint2 { unsigned x, y; }; struct uint3 { unsigned x, y, z; }; struct uint4 { unsigned x, y, z, w; };
struct uchar4 { unsigned char x, y, z, w; };
inline float2 make_float2(ref_real x, ref_real y) { return float2(x, y); }
inline float3 make_float3(ref_real x, ref_real y, ref_real z) { float3 r; r.x = x; r.y = y; r.z = z; return r; }
inline float4 make_float4(ref_real x, ref_real y, ref_real z, ref_real w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
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
inline ref_real __shfl_down(ref_real v, int, int) { return v; }
inline ref_real __int_as_float(unsigned i) { float f; memcpy(&f, &i, 4); return f; }
"""

# Shared by the three drivers: input reading, output writing and the driver's own preconditioned CG (x0 = 0, dots summed in double).
PRELUDE = r"""
#include <cmath>
#include <math.h>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include <iostream>
#include <algorithm>
#include <functional>
#include "cuda_runtime.h"
#if REF_WIDE
#define float double
#define sqrtf sqrt
#define fabsf fabs
#define sinf sin
#define cosf cos
#define expf exp
#define powf pow
#define fminf fmin
#define fmaxf fmax
#endif
%(includes)s
typedef std::vector<double> vec;
static FILE* fin; static FILE* fout;
static vec rd(size_t n) { vec v(n); if (fread(v.data(), 8, n, fin) != n) { fprintf(stderr, "short input\n"); exit(1); } return v; }
static int rdi() { int i; if (fread(&i, 4, 1, fin) != 1) exit(1); return i; }
static std::vector<int> rdiv(size_t n) { std::vector<int> v(n); if (n && fread(v.data(), 4, n, fin) != n) exit(1); return v; }
static void wr(const vec& v) { fwrite(v.data(), 8, v.size(), fout); }
static void wr1(double d) { fwrite(&d, 8, 1, fout); }
static double dotv(const vec& a, const vec& b) { double s = 0; for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i]; return s; }
// k steps of preconditioned CG on A x = b from x = 0; writes x_1 .. x_k.  Opt's PCG preconditions with 1 / (1 + sqrt(P))^2 of its J^T J
// diagonal P (Ceres' guarded inverse) or not at all; the comparator's A is s J^T J, so the same iterates follow from M = g(diag / s) / s with
// the comparator's own diagonal.  s = 0: no preconditioner.
static void cg(const std::function<vec(const vec&)>& A, const vec& b, const vec& diag, double s, int k) {
    size_t n = b.size();
    vec pre(n, 1.0);
    if (s > 0) for (size_t i = 0; i < n; ++i) { double g = 1.0 + std::sqrt(diag[i] / s); pre[i] = 1.0 / (g * g) / s; }
    vec x(n, 0.0), r = b, z(n), p(n);
    for (size_t i = 0; i < n; ++i) z[i] = pre[i] * r[i];
    p = z;
    double rz = dotv(r, z);
    for (int it = 0; it < k; ++it) {
        vec Ap = A(p);
        double alpha = rz / dotv(p, Ap);
        for (size_t i = 0; i < n; ++i) { x[i] += alpha * p[i]; r[i] -= alpha * Ap[i]; z[i] = pre[i] * r[i]; }
        double rzn = dotv(r, z), beta = rzn / rz; rz = rzn;
        for (size_t i = 0; i < n; ++i) p[i] = z[i] + beta * p[i];
        wr(x);
    }
}
"""

POISSON = r"""
int main(int argc, char** argv) {
    fin = fopen(argv[1], "rb"); fout = fopen(argv[2], "wb");
    const int W = rdi(), H = rdi(), N = W * H;
    vec X = rd(4 * N), T = rd(4 * N), M = rd(N), v = rd(4 * N);
    std::vector<float4> x(N), t(N), p(N), delta(N), pre(N); std::vector<float> mask(N);
    for (int i = 0; i < N; ++i) { x[i] = make_float4(X[4*i], X[4*i+1], X[4*i+2], X[4*i+3]); t[i] = make_float4(T[4*i], T[4*i+1], T[4*i+2], T[4*i+3]); mask[i] = M[i]; }
    SolverInput in; in.N = N; in.width = W; in.height = H;
    SolverState st; memset(&st, 0, sizeof st);
    st.d_x = x.data(); st.d_target = t.data(); st.d_mask = mask.data(); st.d_p = p.data(); st.d_delta = delta.data(); st.d_precondioner = pre.data();
    SolverParameters pr; pr.nNonLinearIterations = 1; pr.nLinIterations = 1;
    double F = 0;
    for (int i = 0; i < N; ++i) F += (double)evalFDevice(i, in, st, pr);
    wr1(F);
    vec b(4 * N, 0.0), P(4 * N, 0.0);                       // rows of masked pixels are not unknowns: left 0
    for (int i = 0; i < N; ++i) if (mask[i] == 0) {
        float4 r = evalMinusJTFDevice(i, in, st, pr);
        b[4*i] = r.x; b[4*i+1] = r.y; b[4*i+2] = r.z; b[4*i+3] = r.w;
        P[4*i] = pre[i].x; P[4*i+1] = pre[i].y; P[4*i+2] = pre[i].z; P[4*i+3] = pre[i].w;
    }
    auto A = [&](const vec& q) {
        for (int i = 0; i < N; ++i) p[i] = make_float4(q[4*i], q[4*i+1], q[4*i+2], q[4*i+3]);
        vec o(4 * N, 0.0);
        for (int i = 0; i < N; ++i) if (mask[i] == 0) { float4 r = applyJTJDevice(i, in, st, pr); o[4*i] = r.x; o[4*i+1] = r.y; o[4*i+2] = r.z; o[4*i+3] = r.w; }
        return o;
    };
    wr(b); wr(A(v)); wr(P);
    cg(A, b, P, 0.0, 3);                                     // poisson.t: UsePreconditioner(false)
    return 0;
}
"""

ARAP = r"""
int main(int argc, char** argv) {
    fin = fopen(argv[1], "rb"); fout = fopen(argv[2], "wb");
    const int N = rdi();
    std::vector<int> cnt = rdiv(N), off = rdiv(N); const int E = rdi(); std::vector<int> nbr = rdiv(E);
    vec wt = rd(2), O = rd(3 * N), Ang = rd(3 * N), U = rd(3 * N), C = rd(3 * N), v = rd(6 * N);
    std::vector<float3> x(N), a(N), t(N), u(N), p(N), pA(N), delta(N), deltaA(N), pre(N), preA(N);
    for (int i = 0; i < N; ++i) {
        x[i] = make_float3(O[3*i], O[3*i+1], O[3*i+2]); a[i] = make_float3(Ang[3*i], Ang[3*i+1], Ang[3*i+2]); u[i] = make_float3(U[3*i], U[3*i+1], U[3*i+2]);
        // no constraint: the header's MINF sentinel (the device build's -inf; what MINF expands to here)
        t[i] = std::isfinite(C[3*i]) ? make_float3(C[3*i], C[3*i+1], C[3*i+2]) : make_float3(MINF, MINF, MINF);
    }
    SolverInput in; in.N = N; in.d_numNeighbours = cnt.data(); in.d_neighbourOffset = off.data(); in.d_neighbourIdx = nbr.data();
    SolverState st; memset(&st, 0, sizeof st);
    st.d_x = x.data(); st.d_a = a.data(); st.d_target = t.data(); st.d_urshape = u.data(); st.d_p = p.data(); st.d_pA = pA.data();
    st.d_delta = delta.data(); st.d_deltaA = deltaA.data(); st.d_precondioner = pre.data(); st.d_precondionerA = preA.data();
    SolverParameters pr; pr.weightFitting = wt[0]; pr.weightRegularizer = wt[1]; pr.nNonLinearIterations = 1; pr.nLinIterations = 1;
    double F = 0;
    for (int i = 0; i < N; ++i) F += (double)evalFDevice(i, in, st, pr);
    wr1(F);
    vec b(6 * N), P(6 * N);                                  // Opt's layout: [Offset 3N | Angle 3N]
    for (int i = 0; i < N; ++i) {
        float3 bA; float3 r = evalMinusJTFDevice(i, in, st, pr, bA);
        b[3*i] = r.x; b[3*i+1] = r.y; b[3*i+2] = r.z; b[3*N+3*i] = bA.x; b[3*N+3*i+1] = bA.y; b[3*N+3*i+2] = bA.z;
        P[3*i] = pre[i].x; P[3*i+1] = pre[i].y; P[3*i+2] = pre[i].z; P[3*N+3*i] = preA[i].x; P[3*N+3*i+1] = preA[i].y; P[3*N+3*i+2] = preA[i].z;
    }
    auto A = [&](const vec& q) {
        for (int i = 0; i < N; ++i) { p[i] = make_float3(q[3*i], q[3*i+1], q[3*i+2]); pA[i] = make_float3(q[3*N+3*i], q[3*N+3*i+1], q[3*N+3*i+2]); }
        vec o(6 * N);
        for (int i = 0; i < N; ++i) {
            float3 rA; float3 r = applyJTJDevice(i, in, st, pr, rA);
            o[3*i] = r.x; o[3*i+1] = r.y; o[3*i+2] = r.z; o[3*N+3*i] = rA.x; o[3*N+3*i+1] = rA.y; o[3*N+3*i+2] = rA.z;
        }
        return o;
    };
    wr(b); wr(A(v)); wr(P);
    vec dg(6 * N);
    for (int i = 0; i < 6 * N; ++i) dg[i] = 1.0 / P[i];      // the comparator's preconditioner is 1 / diag(A)
    cg(A, b, dg, 2.0, 3);                                    // A = 2 J^T J
    return 0;
}
"""

SFS = r"""
int main(int argc, char** argv) {
    fin = fopen(argv[1], "rb"); fout = fopen(argv[2], "wb");
    const int W = rdi(), H = rdi(), N = W * H;
    vec sc = rd(16), X = rd(N), D = rd(N), I = rd(N), v = rd(N);
    std::vector<unsigned char> mR(N), mC(N);
    if (fread(mR.data(), 1, N, fin) != (size_t)N || fread(mC.data(), 1, N, fin) != (size_t)N) return 1;
    std::vector<float> x(N), d(N), im(N), p(N, 0), delta(N), L(9), BI(N, 0), B0(N, 0), B1(N, 0), B2(N, 0);
    for (int i = 0; i < N; ++i) { x[i] = X[i]; d[i] = D[i]; im[i] = I[i]; }
    for (int k = 0; k < 9; ++k) L[k] = sc[7 + k];
    SolverInput in; memset(&in, 0, sizeof in); in.N = N; in.width = W; in.height = H;
    in.d_targetIntensity = im.data(); in.d_targetDepth = d.data(); in.d_maskEdgeMapR = mR.data(); in.d_maskEdgeMapC = mC.data(); in.d_litcoeff = L.data();
    in.calibparams.fx = sc[3]; in.calibparams.fy = sc[4]; in.calibparams.ux = sc[5]; in.calibparams.uy = sc[6];
    SolverParameters pr; memset(&pr, 0, sizeof pr);
    pr.weightFitting = sc[0]; pr.weightRegularizer = sc[1]; pr.weightShading = sc[2]; pr.weightShadingStart = sc[2];
    bool* guard = new bool[N]();
    SolverState st; memset(&st, 0, sizeof st);
    st.d_x = x.data(); st.d_p = p.data(); st.d_delta = delta.data(); st.B_I = BI.data(); st.B_I_dx0 = B0.data(); st.B_I_dx1 = B1.data(); st.B_I_dx2 = B2.data(); st.pguard = guard;
    // the precompute pass, on the pixels one in from the left/top and three in from the right/bottom: shading error and its three
    // depth derivatives from the header's own calShading2depthGradCompute, and the Laplacian guard -- the depth and its four
    // neighbours are valid and each neighbour lies within DEPTH_DISCONTINUITY_THRE of the centre
    for (int py = 1; py < H - 2; ++py) for (int px = 1; px < W - 2; ++px) {
        const int i = py * W + px;
        float4 g = calShading2depthGradCompute(st, px, py, in);
        B0[i] = g.x; B1[i] = g.y; B2[i] = g.z; BI[i] = g.w;
        const float c = x[i], nb[4] = {x[i - 1], x[i + 1], x[i - W], x[i + W]};
        bool ok = IsValidPoint(c);
        for (int k = 0; k < 4; ++k) ok = ok && IsValidPoint(nb[k]) && std::fabs(c - nb[k]) < DEPTH_DISCONTINUITY_THRE;
        guard[i] = ok;
    }
    double F = 0;
    for (int i = 0; i < N; ++i) F += (double)evalFDevice(i, in, st, pr);
    wr1(F);
    vec b(N);
    for (int i = 0; i < N; ++i) { float pre; b[i] = evalMinusJTFDevice(i, in, st, pr, pre); }
    auto A = [&](const vec& q) {
        for (int i = 0; i < N; ++i) p[i] = q[i];
        vec o(N);
        for (int i = 0; i < N; ++i) o[i] = applyJTJDevice(i, in, st, pr);
        return o;
    };
    // The stencil of applyJTJ reaches at most 2 pixels in x and in y: check it on every unit vector whose stencil stays inside the
    // image, then read the diagonal off 25 probes, one per class (x mod 5, y mod 5).
    int radius = 0;
    vec e(N, 0.0);
    for (int j = 0; j < N; ++j) {
        e[j] = 1.0; vec c = A(e); e[j] = 0.0;
        for (int i = 0; i < N; ++i) if (c[i] != 0.0) radius = std::max(radius, std::max(std::abs(i % W - j % W), std::abs(i / W - j / W)));
    }
    vec diag(N, 0.0);
    for (int cy = 0; cy < 5; ++cy) for (int cx = 0; cx < 5; ++cx) {
        vec q(N, 0.0);
        for (int i = 0; i < N; ++i) if (i % W % 5 == cx && i / W % 5 == cy) q[i] = 1.0;
        vec c = A(q);
        for (int i = 0; i < N; ++i) if (q[i] != 0.0) diag[i] = c[i];
    }
    wr(b); wr(A(v)); wr(diag); wr1(radius);
    cg(A, b, diag, 0.0, 3);                                  // no UsePreconditioner in shape_from_shading.t: Opt's default is none
    return 0;
}
"""

ENERGIES = {
    # name: (source dir under examples/, includes, driver body)
    "poisson": ("poisson_image_editing/src", ["WarpingSolverState.h", "WarpingSolverParameters.h", "WarpingSolverEquations.h"], POISSON),
    "arap": ("arap_mesh_deformation/src", ["WarpingSolverState.h", "WarpingSolverParameters.h", "WarpingSolverEquations.h"], ARAP),
    "sfs": ("shape_from_shading/src", ["SFSSolverState.h", "SFSSolverParameters.h", "SFSSolverEquations.h"], SFS),
}


def _compile(ref, energy, wide, tmp):
    sub, incs, body = ENERGIES[energy]
    hdr = os.path.join(ref, "examples", sub)
    d = os.path.join(tmp, f"{energy}_{'wide' if wide else 'float'}")
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "cuda_runtime.h"), "w").write(STANDIN_REAL)
    src = PRELUDE % {"includes": "\n".join(f'#include "{os.path.join(hdr, h)}"' for h in incs)} + body
    open(os.path.join(d, "drv.cpp"), "w").write(src)
    exe = os.path.join(d, "drv")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-w", "-fpermissive", "-ffp-contract=off", f"-DREF_REAL={'double' if wide else 'float'}",
                           f"-DREF_WIDE={int(wide)}", f"-I{d}", f"-I{hdr}", os.path.join(d, "drv.cpp"), "-o", exe])
    return exe


def _blob_poisson(P, v):
    W, H = P.dims
    return [np.array([W, H], np.int32), P.params[0], P.params[1], P.params[2], v]


def _blob_arap(P, v):
    N = P.dims[0]
    heads, tails = np.asarray(P.params[7]), np.asarray(P.params[8])
    assert np.all(np.diff(heads) >= 0), "the comparator walks per-vertex neighbour lists: edges must be grouped by head vertex"
    pairs = set(zip(heads.tolist(), tails.tolist()))
    assert all((t, h) in pairs for h, t in pairs), "the comparator cannot express an asymmetric edge list"
    cnt = np.bincount(heads, minlength=N).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    w = np.array([float(P.params[0]) ** 2, float(P.params[1]) ** 2])      # weightFitting = w_fitSqrt^2
    return [np.array([N], np.int32), cnt, off, np.array([len(tails)], np.int32), tails.astype(np.int32), w, P.params[2], P.params[3], P.params[4], P.params[5], v]


def _blob_sfs(P, v):
    W, H = P.dims
    sc = np.array([float(P.params[k]) for k in range(16)])
    return [np.array([W, H], np.int32), sc, P.params[16], P.params[17], P.params[18], v, P.params[19], P.params[20]]


def _run(exe, parts, tmp, n, energy):
    blob, out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(blob, "wb") as f:
        for a in parts:
            a = np.ascontiguousarray(a)
            f.write(a.tobytes() if a.dtype.kind in "iu" else a.astype(np.float64).tobytes())
    subprocess.check_call([exe, blob, out])
    raw = np.frombuffer(open(out, "rb").read(), dtype=np.float64)
    res, pos = {"F": raw[0]}, 1
    names = ["b", "jtj_v", "diag", "radius", "x1", "x2", "x3"] if energy == "sfs" else ["b", "jtj_v", "pre", "x1", "x2", "x3"]
    for k in names:
        m = 1 if k == "radius" else n
        res[k] = raw[pos] if m == 1 else raw[pos:pos + m].copy()
        pos += m
    assert pos == raw.size
    return res


def comparator_cases(ref):
    import reference_cases as rc
    with tempfile.TemporaryDirectory() as tmp:
        exes = {(e, w): _compile(ref, e, w, tmp) for e in ENERGIES for w in (False, True)}
        for name in rc.CASES:
            energy = name.split("_")[0]
            P = rc.problem(name)
            v = rc.probe_vector(P, name)
            parts = {"poisson": _blob_poisson, "arap": _blob_arap, "sfs": _blob_sfs}[energy](P, v)
            fl = _run(exes[(energy, False)], parts, tmp, v.size, energy)
            wd = _run(exes[(energy, True)], parts, tmp, v.size, energy)
            # the widened build is kept only if it reproduces the float build to float rounding, element by element
            for k in fl:
                a, b = np.asarray(fl[k]), np.asarray(wd[k])
                scale = max(float(np.max(np.abs(b))), 1e-300)
                err = float(np.max(np.abs(a - b))) / scale
                print(f"{name:22s} {k:6s} float vs widened: {err:.2e}")
                assert err < (1e-4 if k in ("x1", "x2", "x3") else 2e-5), (name, k, err)
            out = {"v": v, "checksums": rc.checksums(P, v), "F_float": np.float64(fl["F"])}
            for k, val in wd.items():
                out[k] = np.float64(val) if np.ndim(val) == 0 else val
            np.savez_compressed(rc.fixture_path(name), **out)
            print(name, os.path.getsize(rc.fixture_path(name)), "bytes")


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
    comparator_cases(a.reference)
