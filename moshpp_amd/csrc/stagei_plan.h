// Host-side planning of moshii_stagei_core (stagei.hip): the column / row layout of one evaluation, the pose columns and arrow-solver
// tables of a round, and Powell's dogleg over a small problem interface.  Pure arithmetic -- C++17 and standard headers only, no HIP
// types, no environment, no globals -- so that it is tested on its own (tests/test_stagei_plan.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace stagei_plan {

inline int up16(int c) { return (c + 15) & ~15; }

// What one evaluation is made of.  shape_free: the shape columns exist (always in shared mode; per-frame expressions only in the detailed
// rounds).  npid / nfinger / nface: free pose columns per frame, finger rows per frame, face-pose rows per frame.  prior_rows: rows of
// the pose prior per frame (npose + 1 with a mixture, else 0).
struct Facts { int F, M, nobs, nb, per_frame, shape_free, npid, nfinger, nface, prior_rows, nhead_rows; };

// Columns [trans 3F | latent markers 3M | pose F npid | shape nsh], pitch ldn; rows [data | prior | init | beta | surf | poseH | head |
// poseF].  fs / ns / nsp: per-frame and shared unknowns of the arrow solver, and the pitch of its Y.
struct Layout {
    int nsh, n, ldn, o_ml, o_pose, o_b;
    int r_data, r_prior, r_init, r_beta, r_surf, r_poseH, r_head, r_poseF, R;
    int fs, ns, nsp;
};

// no_prior: the prior rows are left out (rigid round; the frozen-attachment evaluation, which also has npid = 0).  rigid (the extra
// rigid adjustment, npid = 3): n = 6 F with pitch ld_rigid, the latent-marker and shape columns parked behind column n (written, never
// read: the products take n columns of a row of ldn).
inline Layout layout(const Facts& k, bool rigid = false, bool no_prior = false, int ld_rigid = 0) {
    Layout l;
    l.nsh = k.per_frame ? (k.shape_free ? k.F * k.nb : 0) : k.nb;
    l.n = 3 * k.F + 3 * k.M + k.F * k.npid + l.nsh; l.ldn = up16(l.n);
    l.o_ml = 3 * k.F; l.o_pose = 3 * k.F + 3 * k.M; l.o_b = l.o_pose + k.F * k.npid;
    if (rigid) { l.n = 6 * k.F; l.ldn = ld_rigid; l.o_pose = 3 * k.F; l.o_ml = 6 * k.F; l.o_b = 6 * k.F + 3 * k.M; }
    l.r_data = 0; l.r_prior = 3 * k.nobs; l.r_init = l.r_prior + (no_prior ? 0 : k.F * k.prior_rows);
    l.r_beta = l.r_init + 3 * k.M; l.r_surf = l.r_beta + l.nsh; l.r_poseH = l.r_surf + k.M; l.r_head = l.r_poseH + k.F * k.nfinger;
    l.r_poseF = l.r_head + 3 * k.nhead_rows; l.R = l.r_poseF + k.F * k.nface;
    l.fs = 3 + k.npid + ((k.per_frame && k.shape_free) ? k.nb : 0); l.ns = 3 * k.M + (k.per_frame ? 0 : k.nb); l.nsp = up16(l.ns);
    return l;
}

// The largest problem of the rounds, for sizing: everything free, the pose ids counted before duplicates are removed.
inline Layout layout_max(Facts k, int n_pose_ids, int n_finger, int n_face) {
    k.shape_free = 1; k.npid = n_pose_ids + n_finger + n_face; k.nfinger = n_finger; k.nface = n_face;
    return layout(k);
}

// The free pose variables of a round, sorted and unique: the root alone in the rigid round, else pose_ids, plus the fingers and the
// face ids (n_face = 0 unless expressions are per frame) in the detailed (last two) rounds.  colmap[NP]: column inside a frame's block, -1 if frozen.
struct PoseCols { std::vector<int> pose_ids, finger_ids, colmap; int nface = 0; };
inline PoseCols pose_columns(int NP, const int* pose_ids, int n_pose_ids, const int* finger_ids, int n_finger, const int* face_ids, int n_face,
                             bool rigid, bool detailed) {
    PoseCols c;
    if (rigid) c.pose_ids = {0, 1, 2};
    else c.pose_ids.assign(pose_ids, pose_ids + n_pose_ids);
    if (detailed) c.finger_ids.assign(finger_ids, finger_ids + n_finger);
    c.pose_ids.insert(c.pose_ids.end(), c.finger_ids.begin(), c.finger_ids.end());
    c.nface = detailed ? n_face : 0;
    if (c.nface) c.pose_ids.insert(c.pose_ids.end(), face_ids, face_ids + c.nface);
    std::sort(c.pose_ids.begin(), c.pose_ids.end());
    c.pose_ids.erase(std::unique(c.pose_ids.begin(), c.pose_ids.end()), c.pose_ids.end());
    c.colmap.assign(NP, -1);
    for (size_t i = 0; i < c.pose_ids.size(); ++i) c.colmap[c.pose_ids[i]] = (int)i;
    return c;
}

// Arrow solver: fcols[F][fs] the columns of frame f's block (trans, pose, per-frame shape), scols[ns] the shared ones (latent markers, shared shape).
inline void arrow_tables(const Facts& k, const Layout& l, std::vector<int>& fcols, std::vector<int>& scols) {
    fcols.resize((size_t)k.F * l.fs); scols.resize(l.ns);
    for (int f = 0; f < k.F; ++f) {
        int* fc = fcols.data() + (size_t)f * l.fs;
        for (int c = 0; c < 3; ++c) fc[c] = 3 * f + c;
        for (int c = 0; c < k.npid; ++c) fc[3 + c] = l.o_pose + f * k.npid + c;
        for (int e = 0; e < l.fs - 3 - k.npid; ++e) fc[3 + k.npid + e] = l.o_b + f * k.nb + e;
    }
    for (int i = 0; i < 3 * k.M; ++i) scols[i] = l.o_ml + i;
    for (int e = 0; e < l.ns - 3 * k.M; ++e) scols[3 * k.M + e] = l.o_b + e;
}

typedef std::vector<double> Vec;
inline double nrm2(const Vec& v) { double s = 0; for (double x : v) s += x * x; return std::sqrt(s); }
inline double dotv(const Vec& a, const Vec& b) { double s = 0; for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i]; return s; }
inline double norminf(const Vec& v) { double s = 0; for (double t : v) s = std::max(s, std::fabs(t)); return s; }

struct DoglegControl { double e1 = 1e-15, e2 = 1e-15, e3 = 0.0, delta0 = 0.5; int maxiter = 200; };
// which way the trial steps went and why the loop ended (for the tests)
struct DoglegTrace { int cauchy = 0, gauss_newton = 0, interpolated = 0, rejected = 0, stop_e1 = 0, stop_e2 = 0, stop_e3 = 0, stop_maxiter = 0; };

// Powell's dogleg on sum r^2 (chumpy minimize_dogleg as restated in oracle/stageii_oracle.py:minimize_dogleg); returns the outer
// iterations, x in place.  Problem:
//   double eval(const Vec& x, bool want_J)   SSE at x (with want_J the Jacobian is kept for normal_eq)
//   void normal_eq(Vec& g)                   A = J^T J, g = -J^T r at the last eval(., true)
//   void Ax(const Vec& v, Vec& out)          A . v
//   void gn_step(Vec& dgn)                   A dgn = g (asked at most once per normal_eq)
template <class Problem>
int dogleg(Problem& prob, Vec& x, const DoglegControl& ctl, DoglegTrace* trace = nullptr) {
    DoglegTrace local;
    DoglegTrace& tr = trace ? *trace : local;
    const int n = (int)x.size();
    const double e1 = ctl.e1, e2 = ctl.e2, e3 = ctl.e3;
    Vec g, dsd, dgn, ddl, tmp, Ag, xt;
    double sse = prob.eval(x, true);
    prob.normal_eq(g);
    double delta = ctl.delta0;
    bool done = false;
    int iteration = 0;
    if (norminf(g) < e1) { done = true; tr.stop_e1++; }
    while (!done) {
        ++iteration;
        // |J g|^2 = g^T A g
        prob.Ax(g, Ag);
        double gg = dotv(g, g), gAg = dotv(g, Ag);
        dsd = g;
        for (double& t : dsd) t *= gg / gAg;
        bool have_gn = false;
        while (true) {
            double nsd = nrm2(dsd);
            if (nsd >= delta) { ddl = dsd; for (double& t : ddl) t *= delta / nsd; tr.cauchy++; }
            else {
                if (!have_gn) { prob.gn_step(dgn); have_gn = true; }
                double ngn = nrm2(dgn);
                if (ngn <= delta) { ddl = dgn; tr.gauss_newton++; }
                else {
                    double dsq = delta * delta, sq_sd = nsd * nsd, dd = 0, dsdd = 0;
                    for (int i = 0; i < n; ++i) { double df = dgn[i] - dsd[i]; dd += df * df; dsdd += df * dsd[i]; }
                    double gs = dotv(dgn, dsd);
                    double pnow = dd * dsq + gs * gs - ngn * ngn * sq_sd;
                    double beta = (dsq - sq_sd) / (dsdd + std::sqrt(pnow));
                    ddl.resize(n);
                    for (int i = 0; i < n; ++i) ddl[i] = dsd[i] + beta * (dgn[i] - dsd[i]);
                    tr.interpolated++;
                }
            }
            double step = nrm2(ddl);
            bool improved = false;
            if (step <= e2 * nrm2(x)) { done = true; tr.stop_e2++; }
            else {
                xt = x;
                for (int i = 0; i < n; ++i) xt[i] += ddl[i];
                const double sse_new = prob.eval(xt, false);
                double rho = sse - sse_new;
                if (rho > 0) {
                    prob.Ax(ddl, tmp);
                    rho = rho / (2.0 * dotv(g, ddl) - dotv(ddl, tmp));
                }
                improved = rho > 0;
                if (improved) {
                    x = xt;
                    if (e3 > 0 && (sse - sse_new) / sse < e3) { done = true; tr.stop_e3++; }
                    else {
                        sse = prob.eval(x, true);
                        prob.normal_eq(g);
                        if (norminf(g) < e1) { done = true; tr.stop_e1++; }
                    }
                } else tr.rejected++;
                if (rho > 0.9) delta = std::max(delta, 2.5 * step);
                else if (rho < 0.05) delta *= 0.25;
                if (delta <= e2 * nrm2(x)) { done = true; tr.stop_e2++; }
            }
            if (done || improved) break;
        }
        if (iteration >= ctl.maxiter) { if (!done) tr.stop_maxiter++; done = true; }
    }
    return iteration;
}

}  // namespace stagei_plan
