// The scalars of a flat PCGStep2 + PCGStep3 pass (graph_pcg.h), included at the top of arap_flatStepPlanes and ge_flatStep: declares alpha, beta and restart from the
// kernel's own LM, L (LmStep<T>), scratch (4 * (blockDim / 64 + 1) doubles) and the partial sums aNumP / nNum, aDenP / nDen, s2P / n2, s3P / n3 of the previous gather.
// alpha = aNum / aDen and beta = max(aNum - 2 alpha s2 + alpha^2 s3, 0) / aNum, all sums in double, with the reference's guards: the values of onchip_sync.h's ocAlpha /
// ocBeta.  After a split residual reset only PCGStep3's beta = sum bNum / sum bDen.
// Included text and not a function: with the two sumPartialsN behind a function boundary -- or with ocAlpha / ocBeta in their place -- the compiler hoists and converts
// differently in the Levenberg-Marquardt kernels; the arithmetic is the same, the instructions are not (profiles/graph_shared_text.md).
    T alpha, beta;
    const bool restart = LM && L.afterReset;
    if (restart) {
        const double* const ps[2] = {L.bNumP, L.bDenP}; const int ns[2] = {L.nbNum, L.nbDen}; double o2[2];
        sumPartialsN<2>(ps, ns, scratch, o2);
        const T bNum = (T)o2[0], bDen = (T)o2[1];
        alpha = T(0); beta = (bDen > T(0)) ? bNum / bDen : T(0);                            // PCGStep3's guard (solver.t:544-547)
    } else {
        const double* const ps[4] = {aNumP, aDenP, s2P, s3P}; const int ns[4] = {nNum, nDen, n2, n3}; double o4[4];
        sumPartialsN<4>(ps, ns, scratch, o4);
        const T aNum = (T)o4[0], aDen = (T)o4[1];
        alpha = (aDen > T(0)) ? aNum / aDen : T(0);                                          // solver.t:456-459
        const double bNumD = fmax(o4[0] - 2.0 * (double)alpha * o4[2] + (double)alpha * (double)alpha * o4[3], 0.0);
        beta = (aNum > T(0)) ? (T)bNumD / aNum : T(0);                                       // solver.t:544-547
    }
