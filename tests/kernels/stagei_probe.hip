// TEST INFRASTRUCTURE: host launchers for single Stage-I kernels, so that tests/test_stagei_kernels.py can hold each one to a
// high-precision reference.  The product source is included UNCHANGED (its kernels live in an anonymous namespace: including the file is
// how a test reaches them); tests/kernels/build_probe.py compiles this file with hipcc for gfx950 (the flags moshpp_amd/build.py gives
// stagei.hip) or with g++ against tests/emu/fakehip.  Never linked into libmoshii.
//
// Every launcher takes host arrays.  An output argument is the WHOLE host buffer, guard bands included: it is uploaded as it is (so the
// device copy carries the caller's sentinels), the kernels get the pointer `PG` elements in, and all of it is copied back -- what the
// kernels wrote outside their range shows up in the guards.  status words are copied both ways without guards.  The factorisation and
// the arrow step are the product's own launch sequences (s1_chol_factor, s1_arrow_reduce, s1_arrow_solve); the single launches follow
// moshii_stagei_core: same grids, threads and dynamic LDS.
// Return: 0, or -1 if a HIP call failed.
#include "../../moshpp_amd/csrc/stagei.hip"

#define PG 64     // guard elements on either side of every output buffer (tests/test_stagei_kernels.py: GUARD)

namespace {
struct Probe {
    std::vector<void*> dev;
    std::vector<std::pair<void*, std::pair<const void*, size_t>>> back;   // (host, (device, bytes)) copied back by finish()
    bool ok = true;
    template <class T> T* in(const T* h, size_t count) {           // read-only input
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) { ok = false; return nullptr; }
        dev.push_back(q);
        if (count && hipMemcpy(q, h, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) ok = false;
        return (T*)q;
    }
    template <class T> T* out(T* h, size_t count) {                // [PG | count | PG] both ways; the kernels see the middle
        T* q = in<T>(h, count + 2 * PG);
        if (q) back.push_back({(void*)h, {(const void*)q, (count + 2 * PG) * sizeof(T)}});
        return q ? q + PG : nullptr;
    }
    template <class T> T* io(T* h, size_t count) {                 // small in-out words (status), no guards
        T* q = in<T>(h, count);
        if (q) back.push_back({(void*)h, {(const void*)q, count * sizeof(T)}});
        return q;
    }
    int finish() {
        if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) ok = false;
        for (auto& b : back)
            if (ok && hipMemcpy(b.first, b.second.first, b.second.second, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
        for (void* q : dev) hipFree(q);
        return ok ? 0 : -1;
    }
};

}  // namespace

extern "C" {

int probe_tpb() { return S1_TPB; }

// flags = k_s1_nzflags(J) then A = J^T J by k_s1_syrk (the normal equations).  given_flags = 1: the flags are the caller's (the Schur
// path's all-ones form on Y) and k_s1_nzflags is not run.  A: n x n, flags: ceil(R / 32) x ceil(n / 32), both guarded.
int probe_syrk(const double* J, int R, int n, int ldn, int given_flags, int* flags, double* A) {
    Probe pr;
    const int nt = (n + S1_T - 1) / S1_T, nrc = (R + S1_T - 1) / S1_T;
    const double* dJ = pr.in(J, (size_t)R * ldn);
    int* dF = pr.out(flags, (size_t)nrc * nt);
    double* dA = pr.out(A, (size_t)n * n);
    if (!pr.ok) return pr.finish();
    if (!given_flags) LAUNCH(k_s1_nzflags, nrc, nt, 256, 0, dJ, R, n, ldn, dF);
    LAUNCH(k_s1_syrk, nt, nt, 256, 0, dJ, R, n, ldn, dA, dF);
    return pr.finish();
}

// y = sign J^T r through k_s1_gemv_t (partials [S1_GT_CHUNKS][n]) and k_s1_gemv_t_sum
int probe_gemv_t(const double* J, const double* r, int R, int n, int ldn, double sign, double* part, double* y) {
    Probe pr;
    const double* dJ = pr.in(J, (size_t)R * ldn); const double* dr = pr.in(r, (size_t)R);
    double* dP = pr.out(part, (size_t)S1_GT_CHUNKS * n); double* dy = pr.out(y, (size_t)n);
    if (!pr.ok) return pr.finish();
    LAUNCH(k_s1_gemv_t, (n + S1_TPB - 1) / S1_TPB, S1_GT_CHUNKS, S1_TPB, 0, dJ, dr, R, n, ldn, dP);
    LAUNCH(k_s1_gemv_t_sum, (n + S1_TPB - 1) / S1_TPB, 1, S1_TPB, 0, dP, n, sign, dy);
    return pr.finish();
}

// y[rows] = Mx[rows][ld] . x[n]  (k_s1_gemv: the host's A . v)
int probe_gemv(const double* Mx, const double* x, int rows, int n, int ld, double* y) {
    Probe pr;
    const double* dM = pr.in(Mx, (size_t)rows * ld); const double* dx = pr.in(x, (size_t)n);
    double* dy = pr.out(y, (size_t)rows);
    if (!pr.ok) return pr.finish();
    LAUNCH(k_s1_gemv, rows, 1, S1_TPB, 0, dM, dx, n, ld, dy);
    return pr.finish();
}

// A (n x n, in place, guarded) -> its blocked Cholesky factor, dinv (ceil(n / 32) x 32 x 32, guarded) the panels' inverse diagonal
// blocks, x = A^-1 g by k_s1_tri_solve (guarded); status[3] as the solver keeps it (status[1]: a pivot was not positive)
int probe_chol(double* A, int n, double* dinv, const double* g, double* x, int* status) {
    if (n < 1 || n > S1_NMAX) return -1;
    Probe pr;
    double* dA = pr.out(A, (size_t)n * n);
    double* dD = pr.out(dinv, (size_t)((n + S1_PB - 1) / S1_PB) * S1_PB * S1_PB);
    const double* dg = pr.in(g, (size_t)n);
    double* dx = pr.out(x, (size_t)n);
    int* dS = pr.io(status, 3);
    if (!pr.ok) return pr.finish();
    s1_chol_factor(dA, n, dD, dS, 0);
    LAUNCH(k_s1_tri_solve, 1, 1, S1_CHOL_TPB, 0, dA, n, dD, dg, dx);
    return pr.finish();
}

// The arrow-structured Gauss-Newton step of moshii_stagei_core on the frames [fbase, fbase + nown) of F, both halves as the solver runs
// them (no rank sum in between): k_s1_elim, k_s1_elim_y, the SYRK of Y (all-ones flags), k_s1_schur_sub; the blocked Cholesky of S,
// k_s1_tri_solve, k_s1_back.  A: n x n (lower part read), g: n, fcols: F x fs, scols: ns.  Outputs (guarded): Linv F x fs x fs, Y F x fs x nsp, z F x fs, T / S ns x ns, h / ds ns, dinv, out n (NOT
// cleared first: the caller's fill shows which entries k_s1_back wrote).
int probe_schur(const double* A, int n, const double* g, const int* fcols, int F, int fs, const int* scols, int ns, int fbase, int nown,
                int scatter_shared, double* Linv, double* Y, double* z, double* T, double* S, double* h, double* dinv, double* ds,
                double* out, int* status) {
    if (fs < 1 || fs > S1_FSMAX || ns < 1 || ns > S1_NMAX || nown < 1 || fbase < 0 || fbase + nown > F) return -1;
    Probe pr;
    const int nsp = (ns + 15) & ~15;
    const double* dA = pr.in(A, (size_t)n * n); const double* dg = pr.in(g, (size_t)n);
    const int* dfc = pr.in(fcols, (size_t)F * fs); const int* dsc = pr.in(scols, (size_t)ns);
    std::vector<int> ones((size_t)((F * fs + S1_T - 1) / S1_T) * ((ns + S1_T - 1) / S1_T), 1);
    const int* d1 = pr.in(ones.data(), ones.size());
    double* dL = pr.out(Linv, (size_t)F * fs * fs); double* dY = pr.out(Y, (size_t)F * fs * nsp); double* dz = pr.out(z, (size_t)F * fs);
    double* dT = pr.out(T, (size_t)ns * ns); double* dS = pr.out(S, (size_t)ns * ns); double* dh = pr.out(h, (size_t)ns);
    double* dD = pr.out(dinv, (size_t)((ns + S1_PB - 1) / S1_PB) * S1_PB * S1_PB); double* dds = pr.out(ds, (size_t)ns);
    double* dout = pr.out(out, (size_t)n);
    int* dst = pr.io(status, 3);
    if (!pr.ok) return pr.finish();
    const S1Arrow a{dA, n, dg, dfc, F, fs, dsc, ns, nsp, d1, dL, dY, dz, dT, dS, dh, dD, dds, dst, fbase, nown};
    s1_arrow_reduce(a, 0);
    s1_arrow_solve(a, dout, false, scatter_shared, 0);
    return pr.finish();
}

// the 8 nearest canonical vertices of every marker (k_s1_knn, grid M) and the attachment triple picked from them (k_s1_pick3, one
// workgroup).  can: V x 3, excl: V bytes, ml: M x 3; cl8: M x 8, cl: M x 3 (guarded); status[3] (status[2]: collinear to the end)
int probe_knn(const double* can, const unsigned char* excl, int V, const double* ml, int M, int* cl8, int* cl, int* status) {
    Probe pr;
    S1Dims d; memset(&d, 0, sizeof(d)); S1Ptr p; memset(&p, 0, sizeof(p));
    d.V = V; d.M = M;
    p.can = pr.in(can, (size_t)3 * V); p.excl = pr.in(excl, (size_t)V); p.ml = pr.in(ml, (size_t)3 * M);
    int* d8 = pr.out(cl8, (size_t)S1_NNK * M); int* d3 = pr.out(cl, (size_t)3 * M);
    p.status = pr.io(status, 3);
    if (!pr.ok) return pr.finish();
    LAUNCH(k_s1_knn, M, 1, S1_TPB, 0, d, p, d8);
    LAUNCH(k_s1_pick3, 1, 1, S1_TPB, 0, d, p, (const int*)d8, d3);
    return pr.finish();
}

// signed distance of every marker to the surface (k_s1_surface, grid M, S1_SURF_TPB threads).  v2f_ptr / v2f: the vertex -> incident
// faces lists moshii_stagei_core builds.  Outputs (guarded): sdist M, tv M x 3, sdp M x 3, sdabc M x 9
int probe_surface(const double* can, int V, const int* faces, int nfaces, const int* v2f_ptr, const int* v2f, const double* ml, int M,
                  double* sdist, int* tv, double* sdp, double* sdabc) {
    Probe pr;
    S1Dims d; memset(&d, 0, sizeof(d)); S1Ptr p; memset(&p, 0, sizeof(p));
    d.V = V; d.M = M; d.nfaces = nfaces;
    p.can = pr.in(can, (size_t)3 * V); p.faces = pr.in(faces, (size_t)3 * nfaces);
    p.v2f_ptr = pr.in(v2f_ptr, (size_t)V + 1); p.v2f = pr.in(v2f, (size_t)3 * nfaces); p.ml = pr.in(ml, (size_t)3 * M);
    p.sdist = pr.out(sdist, (size_t)M); p.tv = pr.out(tv, (size_t)3 * M); p.sdp = pr.out(sdp, (size_t)3 * M); p.sdabc = pr.out(sdabc, (size_t)9 * M);
    if (!pr.ok) return pr.finish();
    LAUNCH(k_s1_surface, M, 1, S1_SURF_TPB, 0, d, p);
    return pr.finish();
}

}  // extern "C"
