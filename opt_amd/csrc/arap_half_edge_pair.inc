// One half-edge pair (v -> u), (u -> v) of a symmetric graph at vertex v, as arap_edges<3> would compute both edges: the body of the walk over a vertex's ELL out-list,
// included by arap_applyEll (energy_graph.hip) and aoApply (arap_onchip.h) inside their `for j` over the batch.  From the enclosing loop: cv (arap_coef of v's angles),
// w = w_reg, wm[j] (w, or 0 beyond v's degree), pv / pav (p and its Angle part at v), u0 (v's entry of U0) and the neighbour's entries nd0[j] / nd1[j] (its p and pa,
// from the dynamic planes or from LDS), nt0[j] / nt1[j] / nu0[j] (static planes); it adds to s0..s2 / s3..s5, the Offset / Angle rows of (J^T J p)(v), and to acc, the
// edge's |J p|^2.  Included text and not a function: behind a function boundary the compiler contracts the sums of products here into other fused multiply-adds, and
// p . A p comes out with other last bits (profiles/graph_shared_text.md).
    const T wj = wm[j];
    const V3<T> np{nd0[j].a, nd0[j].b, nd0[j].c}, npa{nd0[j].d, nd1[j].a, nd1[j].b};
    const V3<T> u{u0.a - nu0[j].a, u0.b - nu0[j].b, u0.c - nu0[j].c}, un{-u.x, -u.y, -u.z};      // U_v - U_u: the subtraction the slots of rounds 3-5 stored
    V3<T> D0, D1, D2;
    arap_cols(cv, u, D0, D1, D2);
    {   // out-edge (v -> u): J p and D_k . J p  (arap_edges<3> with v0 = v)
        const T jx = w * (pv.x - np.x) - w * (D0.x * pav.x + D1.x * pav.y + D2.x * pav.z);
        const T jy = w * (pv.y - np.y) - w * (D0.y * pav.x + D1.y * pav.y + D2.y * pav.z);
        const T jz = w * (pv.z - np.z) - w * (D0.z * pav.x + D1.z * pav.y + D2.z * pav.z);
        s0 += wj * jx; s1 += wj * jy; s2 += wj * jz;
        s3 -= wj * (D0.x * jx + D0.y * jy + D0.z * jz); s4 -= wj * (D1.x * jx + D1.y * jy + D1.z * jz); s5 -= wj * (D2.x * jx + D2.y * jy + D2.z * jz);
        if (wj != T(0)) acc += (double)(jx * jx + jy * jy + jz * jz);              // sum_u p_u (J^T J p)_u of this edge = |J p|^2 (o.t:2117-2122)
    }
    {   // its reverse (u -> v): only its J p reaches this vertex's Offset row
        const ArapCoef<T> cu = arap_coef(nt0[j].a, nt0[j].b, nt0[j].c, nt0[j].d, nt1[j].a, nt1[j].b);
        V3<T> E0, E1, E2;
        arap_cols(cu, un, E0, E1, E2);
        const T jx = w * (np.x - pv.x) - w * (E0.x * npa.x + E1.x * npa.y + E2.x * npa.z);
        const T jy = w * (np.y - pv.y) - w * (E0.y * npa.x + E1.y * npa.y + E2.y * npa.z);
        const T jz = w * (np.z - pv.z) - w * (E0.z * npa.x + E1.z * npa.y + E2.z * npa.z);
        s0 -= wj * jx; s1 -= wj * jy; s2 -= wj * jz;
    }
