"""CPU: the host-side planning of the Stage-I solve (moshpp_amd/csrc/stagei_plan.h: evaluation layout, pose columns, arrow-solver tables,
Powell's dogleg) compiled on its own by g++ -- no HIP, no device.  The layout is held to numbers worked out by hand below, the dogleg to
oracle.stageii_oracle.minimize_dogleg on small analytic least-squares problems written once in the C++ program and once here."""
import os
import subprocess

import numpy as np
import pytest

from oracle import stageii_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include "stagei_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace stagei_plan;

static void show(const char* name, const Layout& l) {
    printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", name, l.nsh, l.n, l.ldn, l.o_ml, l.o_pose, l.o_b, l.r_data, l.r_prior,
           l.r_init, l.r_beta, l.r_surf, l.r_poseH, l.r_head, l.r_poseF, l.R, l.fs, l.ns, l.nsp);
}
static void ints(const char* name, const std::vector<int>& v) { printf("%s", name); for (int i : v) printf(" %d", i); printf("\n"); }
static void cols(const char* name, bool rigid, bool detailed, int n_face) {
    const int pose_ids[] = {0, 1, 2, 5}, finger_ids[] = {5, 8}, face_ids[] = {9};
    const PoseCols c = pose_columns(12, pose_ids, 4, finger_ids, 2, face_ids, n_face, rigid, detailed);
    char key[64];
    snprintf(key, sizeof(key), "%s_pose", name); ints(key, c.pose_ids);
    snprintf(key, sizeof(key), "%s_finger", name); ints(key, c.finger_ids);
    snprintf(key, sizeof(key), "%s_colmap", name); ints(key, c.colmap);
    printf("%s_nface %d\n", name, c.nface);
}

// r(x) and J(x) of the analytic problems (tests/test_stagei_plan.py states the same ones in Python)
struct Problem {
    int kind, m, n, trial = 0, jac = 0;
    Vec r, J, A, g;
    Problem(int kind_) : kind(kind_) { const int ms[] = {2, 4, 6, 3}, ns[] = {2, 4, 3, 2}; m = ms[kind]; n = ns[kind]; }
    void residual(const Vec& x, bool want_J) {
        r.assign(m, 0.0);
        if (want_J) J.assign((size_t)m * n, 0.0);
        if (kind == 0) {            // Rosenbrock's valley, flattened: 1.5 (x1 - x0^2), 1 - x0
            r[0] = 1.5 * (x[1] - x[0] * x[0]); r[1] = 1.0 - x[0];
            if (want_J) { J[0] = -3.0 * x[0]; J[1] = 1.5; J[2] = -1.0; }
        } else if (kind == 1) {     // Powell's singular function
            const double s5 = sqrt(5.0), s10 = sqrt(10.0);
            r[0] = x[0] + 10.0 * x[1]; r[1] = s5 * (x[2] - x[3]); r[2] = (x[1] - 2.0 * x[2]) * (x[1] - 2.0 * x[2]); r[3] = s10 * (x[0] - x[3]) * (x[0] - x[3]);
            if (want_J) {
                J[0] = 1.0; J[1] = 10.0; J[6] = s5; J[7] = -s5; J[9] = 2.0 * (x[1] - 2.0 * x[2]); J[10] = -4.0 * (x[1] - 2.0 * x[2]);
                J[12] = 2.0 * s10 * (x[0] - x[3]); J[15] = -2.0 * s10 * (x[0] - x[3]);
            }
        } else if (kind == 2) {     // exponential fit: x0 exp(-x1 t) + x2 against exact data of (2, 1, 1) at t = 0, 0.5 .. 2.5
            for (int i = 0; i < m; ++i) {
                const double t = 0.5 * i, e = exp(-x[1] * t);
                r[i] = x[0] * e + x[2] - (2.0 * exp(-t) + 1.0);
                if (want_J) { J[3 * i] = e; J[3 * i + 1] = -x[0] * t * e; J[3 * i + 2] = 1.0; }
            }
        } else {                    // two circles and a line: mildly nonlinear, well conditioned
            r[0] = x[0] * x[0] + x[1] * x[1] - 2.0; r[1] = x[0] - x[1]; r[2] = 0.5 * (x[0] + x[1] - 2.0);
            if (want_J) { J[0] = 2.0 * x[0]; J[1] = 2.0 * x[1]; J[2] = 1.0; J[3] = -1.0; J[4] = 0.5; J[5] = 0.5; }
        }
    }
    double eval(const Vec& x, bool want_J) { residual(x, want_J); ++(want_J ? jac : trial); return dotv(r, r); }
    void normal_eq(Vec& g_) {
        A.assign((size_t)n * n, 0.0); g.assign(n, 0.0);
        for (int a = 0; a < n; ++a) {
            for (int b = 0; b < n; ++b) for (int i = 0; i < m; ++i) A[a * n + b] += J[i * n + a] * J[i * n + b];
            for (int i = 0; i < m; ++i) g[a] -= J[i * n + a] * r[i];
        }
        g_ = g;
    }
    void Ax(const Vec& v, Vec& out) { out.assign(n, 0.0); for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) out[a] += A[a * n + b] * v[b]; }
    void gn_step(Vec& dgn) {        // plain Cholesky solve
        Vec L(A);
        for (int j = 0; j < n; ++j) {
            for (int c = 0; c < j; ++c) L[j * n + j] -= L[j * n + c] * L[j * n + c];
            L[j * n + j] = sqrt(L[j * n + j]);
            for (int i = j + 1; i < n; ++i) { for (int c = 0; c < j; ++c) L[i * n + j] -= L[i * n + c] * L[j * n + c]; L[i * n + j] /= L[j * n + j]; }
        }
        dgn = g;
        for (int i = 0; i < n; ++i) { for (int c = 0; c < i; ++c) dgn[i] -= L[i * n + c] * dgn[c]; dgn[i] /= L[i * n + i]; }
        for (int i = n - 1; i >= 0; --i) { for (int c = i + 1; c < n; ++c) dgn[i] -= L[c * n + i] * dgn[c]; dgn[i] /= L[i * n + i]; }
    }
};

// dogleg <name> <kind> <e3> <maxiter> <x0 ...>
static int run_dogleg(int argc, char** argv) {
    Problem pb(atoi(argv[3]));
    DoglegControl ctl;
    ctl.e3 = atof(argv[4]); ctl.maxiter = atoi(argv[5]);
    Vec x;
    for (int i = 6; i < argc; ++i) x.push_back(strtod(argv[i], nullptr));
    DoglegTrace t;
    const int it = dogleg(pb, x, ctl, &t);
    printf("%s %d %d %d %d %d %d %d %d %d %d %d", argv[2], it, pb.trial, pb.jac, t.cauchy, t.gauss_newton, t.interpolated, t.rejected, t.stop_e1, t.stop_e2,
           t.stop_e3, t.stop_maxiter);
    for (double v : x) printf(" %.17g", v);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "dogleg") == 0) return run_dogleg(argc, argv);
    // F = 2, M = 3, nb = 2, four observations (two short of full), five prior rows per frame.  Facts: F M nobs nb per_frame shape_free npid nfinger nface prior_rows nhead_rows
    const Facts shared{2, 3, 4, 2, 0, 1, 0, 0, 0, 5, 0}, framed{2, 3, 4, 2, 1, 0, 0, 0, 0, 5, 0};
    Facts k = shared;
    const Layout mx_shared = layout_max(shared, 4, 2, 0), mx_framed = layout_max(framed, 4, 2, 1);
    k.npid = 4; show("body", layout(k));
    k.nhead_rows = 2; show("head", layout(k)); show("max_head", layout_max(k, 4, 2, 0)); k.nhead_rows = 0;
    k.npid = 6; k.nfinger = 2; show("fingers", layout(k));
    k = shared; k.npid = 3; show("rigid", layout(k, true, true, mx_shared.ldn));
    k = shared; show("frozen", layout(k, false, true));
    k = framed; k.npid = 4; show("framed_body", layout(k));
    k.shape_free = 1; k.npid = 7; k.nfinger = 2; k.nface = 1; show("framed_detailed", layout(k));
    k = framed; show("framed_frozen", layout(k, false, true));
    show("max_shared", mx_shared); show("max_framed", mx_framed);
    cols("cols_body", false, false, 0); cols("cols_detailed", false, true, 0); cols("cols_face", false, true, 1); cols("cols_face_early", false, false, 1);
    cols("cols_rigid", true, false, 1);
    std::vector<int> fcols, scols;
    k = shared; k.npid = 4; arrow_tables(k, layout(k), fcols, scols); ints("fcols_body", fcols); ints("scols_body", scols);
    k = framed; k.shape_free = 1; k.npid = 7; k.nfinger = 2; k.nface = 1; arrow_tables(k, layout(k), fcols, scols); ints("fcols_framed", fcols); ints("scols_framed", scols);
    return 0;
}
'''

FIELDS = ['nsh', 'n', 'ldn', 'o_ml', 'o_pose', 'o_b', 'r_data', 'r_prior', 'r_init', 'r_beta', 'r_surf', 'r_poseH', 'r_head', 'r_poseF', 'R', 'fs', 'ns',
          'nsp']


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp('stagei_plan')
    src, out = d / 'plan.cpp', d / 'plan'
    src.write_text(PROGRAM)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'moshpp_amd', 'csrc'), str(src), '-o', str(out)])
    return str(out)


@pytest.fixture(scope='module')
def plan(exe):
    """The program's output lines, by their first word."""
    return {line.split()[0]: [int(v) for v in line.split()[1:]] for line in subprocess.check_output([exe]).decode().splitlines()}


def _layout(plan, name):
    return dict(zip(FIELDS, plan[name]))


# Worked by hand.  Columns: 3 F = 6 translations, 3 M = 9 latent-marker coordinates from 6, F npid pose columns from 15, the shape block
# behind them.  Rows: 3 * 4 = 12 data rows, F * 5 = 10 prior rows, 9 init rows, nsh beta rows, M = 3 surface rows, F nfinger finger
# rows, 3 nhead_rows head rows, F nface face rows.
LAYOUTS = {
    # 4 pose columns per frame: n = 6 + 9 + 8 + 2 = 25; rows 12 | 10 | 9 | 2 | 3
    'body': dict(nsh=2, n=25, ldn=32, o_ml=6, o_pose=15, o_b=23, r_data=0, r_prior=12, r_init=22, r_beta=31, r_surf=33, r_poseH=36, r_head=36,
                 r_poseF=36, R=36, fs=7, ns=11, nsp=16),
    # ... with 2 head rows: 6 more rows behind the (empty) finger block
    'head': dict(nsh=2, n=25, ldn=32, o_ml=6, o_pose=15, o_b=23, r_data=0, r_prior=12, r_init=22, r_beta=31, r_surf=33, r_poseH=36, r_head=36,
                 r_poseF=42, R=42, fs=7, ns=11, nsp=16),
    # detailed round, two fingers: 6 pose columns, n = 6 + 9 + 12 + 2 = 29; 4 finger rows
    'fingers': dict(nsh=2, n=29, ldn=32, o_ml=6, o_pose=15, o_b=27, r_data=0, r_prior=12, r_init=22, r_beta=31, r_surf=33, r_poseH=36, r_head=40,
                    r_poseF=40, R=40, fs=9, ns=11, nsp=16),
    # rigid round: n = 6 F = 12 at the pitch of the largest round (32), root columns from 6, latent markers parked at 12, shape at 21;
    # no prior rows
    'rigid': dict(nsh=2, n=12, ldn=32, o_ml=12, o_pose=6, o_b=21, r_data=0, r_prior=12, r_init=12, r_beta=21, r_surf=23, r_poseH=26, r_head=26,
                  r_poseF=26, R=26, fs=6, ns=11, nsp=16),
    # frozen attachment: no pose columns, no prior rows: n = 6 + 9 + 2 = 17
    'frozen': dict(nsh=2, n=17, ldn=32, o_ml=6, o_pose=15, o_b=15, r_data=0, r_prior=12, r_init=12, r_beta=21, r_surf=23, r_poseH=26, r_head=26,
                   r_poseF=26, R=26, fs=3, ns=11, nsp=16),
    # per-frame expressions before the detailed rounds: no shape columns or rows, the shared block is the latent markers alone
    'framed_body': dict(nsh=0, n=23, ldn=32, o_ml=6, o_pose=15, o_b=23, r_data=0, r_prior=12, r_init=22, r_beta=31, r_surf=31, r_poseH=34,
                        r_head=34, r_poseF=34, R=34, fs=7, ns=9, nsp=16),
    # ... detailed: 4 + 2 fingers + 1 face id = 7 pose columns, F nb = 4 expression columns: n = 6 + 9 + 14 + 4 = 33; 4 finger, 2 face rows
    'framed_detailed': dict(nsh=4, n=33, ldn=48, o_ml=6, o_pose=15, o_b=29, r_data=0, r_prior=12, r_init=22, r_beta=31, r_surf=35, r_poseH=38,
                            r_head=42, r_poseF=42, R=44, fs=12, ns=9, nsp=16),
    'framed_frozen': dict(nsh=0, n=15, ldn=16, o_ml=6, o_pose=15, o_b=15, r_data=0, r_prior=12, r_init=12, r_beta=21, r_surf=21, r_poseH=24,
                          r_head=24, r_poseF=24, R=24, fs=3, ns=9, nsp=16),
}


@pytest.mark.parametrize('name', sorted(LAYOUTS))
def test_layout(plan, name):
    assert _layout(plan, name) == LAYOUTS[name]


def test_sizing_maxima_bound_every_round(plan):
    """The sizing layout counts the pose ids before duplicates are removed (4 + 2 [+ 1]) and has everything free."""
    assert _layout(plan, 'max_shared') == LAYOUTS['fingers']
    assert _layout(plan, 'max_framed') == LAYOUTS['framed_detailed']
    families = {'max_shared': ['body', 'fingers', 'rigid', 'frozen'], 'max_head': ['head'], 'max_framed': ['framed_body', 'framed_detailed', 'framed_frozen']}
    for mx_name, names in families.items():
        mx = _layout(plan, mx_name)
        for name in names:
            lay = _layout(plan, name)
            assert all(lay[f] <= mx[f] for f in ('n', 'ldn', 'R', 'fs', 'ns', 'nsp', 'nsh')), (mx_name, name)
    rigid = _layout(plan, 'rigid')
    assert rigid['ldn'] == _layout(plan, 'max_shared')['ldn'] and rigid['o_b'] + rigid['nsh'] <= rigid['ldn']      # the parked columns fit the pitch


def test_pose_columns(plan):
    """pose_ids (0, 1, 2, 5), finger_ids (5, 8) -- 5 in both --, face id 9, of 12 pose variables."""
    def colmap(ids):
        return [ids.index(v) if v in ids else -1 for v in range(12)]
    want = {'cols_body': ([0, 1, 2, 5], [], 0), 'cols_detailed': ([0, 1, 2, 5, 8], [5, 8], 0), 'cols_face': ([0, 1, 2, 5, 8, 9], [5, 8], 1),
            'cols_face_early': ([0, 1, 2, 5], [], 0), 'cols_rigid': ([0, 1, 2], [], 0)}
    for name, (ids, fingers, nface) in want.items():
        assert plan[name + '_pose'] == ids and plan[name + '_finger'] == fingers and plan[name + '_nface'] == [nface], name
        assert plan[name + '_colmap'] == colmap(ids), name
    assert plan['cols_detailed_colmap'] == [0, 1, 2, -1, -1, 3, -1, -1, 4, -1, -1, -1]


def test_arrow_tables(plan):
    assert plan['fcols_body'] == [0, 1, 2, 15, 16, 17, 18] + [3, 4, 5, 19, 20, 21, 22]
    assert plan['scols_body'] == list(range(6, 15)) + [23, 24]
    assert plan['fcols_framed'] == [0, 1, 2] + list(range(15, 22)) + [29, 30] + [3, 4, 5] + list(range(22, 29)) + [31, 32]
    assert plan['scols_framed'] == list(range(6, 15))


# ---- the dogleg against the oracle's ------------------------------------------------------------------------------------------------
class _Rosenbrock:
    solution = np.array([1.0, 1.0])

    def r(self, x):
        return np.array([1.5 * (x[1] - x[0] * x[0]), 1.0 - x[0]])

    def J(self, x):
        return np.array([[-3.0 * x[0], 1.5], [-1.0, 0.0]])


class _PowellSingular:
    solution = None         # singular there: only runs that are stopped early

    def r(self, x):
        return np.array([x[0] + 10.0 * x[1], np.sqrt(5.0) * (x[2] - x[3]), (x[1] - 2.0 * x[2]) ** 2, np.sqrt(10.0) * (x[0] - x[3]) ** 2])

    def J(self, x):
        s5, s10 = np.sqrt(5.0), np.sqrt(10.0)
        return np.array([[1.0, 10.0, 0.0, 0.0], [0.0, 0.0, s5, -s5], [0.0, 2.0 * (x[1] - 2.0 * x[2]), -4.0 * (x[1] - 2.0 * x[2]), 0.0],
                         [2.0 * s10 * (x[0] - x[3]), 0.0, 0.0, -2.0 * s10 * (x[0] - x[3])]])


class _ExpFit:
    solution = np.array([2.0, 1.0, 1.0])
    t = 0.5 * np.arange(6)

    def r(self, x):
        return x[0] * np.exp(-x[1] * self.t) + x[2] - (2.0 * np.exp(-self.t) + 1.0)

    def J(self, x):
        e = np.exp(-x[1] * self.t)
        return np.stack([e, -x[0] * self.t * e, np.ones(6)], axis=1)


class _Circles:
    solution = np.array([1.0, 1.0])

    def r(self, x):
        return np.array([x[0] * x[0] + x[1] * x[1] - 2.0, x[0] - x[1], 0.5 * (x[0] + x[1] - 2.0)])

    def J(self, x):
        return np.array([[2.0 * x[0], 2.0 * x[1]], [1.0, -1.0], [0.5, 0.5]])


PROBLEMS = [_Rosenbrock(), _PowellSingular(), _ExpFit(), _Circles()]
# name: (problem, e_3, maxiter, x0)
RUNS = {
    'rosenbrock_far': (0, 0.0, 200, [-1.2, 1.0]),
    'powell_maxiter': (1, 0.0, 6, [3.0, -1.0, 0.0, 1.0]),
    'expfit': (2, 0.0, 200, [1.0, 0.3, 0.0]),
    'circles_near': (3, 0.0, 200, [1.2, 0.9]),
    'circles_far': (3, 0.0, 200, [4.0, -3.0]),
    'circles_e3': (3, 0.5, 200, [4.0, -3.0]),           # the first (Cauchy) step gains less than half
}
TRACE = ['cauchy', 'gauss_newton', 'interpolated', 'rejected', 'stop_e1', 'stop_e2', 'stop_e3', 'stop_maxiter']


def _oracle(run, x0=None):
    kind, e3, maxiter, start = RUNS[run]
    stats = {}
    x = so.minimize_dogleg(PROBLEMS[kind], np.array(start if x0 is None else x0), e_3=e3, delta_0=0.5, maxiter=maxiter, stats=stats)
    return x, stats


@pytest.fixture(scope='module')
def dogleg_runs(exe):
    out = {}
    for run, (kind, e3, maxiter, x0) in RUNS.items():
        words = subprocess.check_output([exe, 'dogleg', run, str(kind), repr(e3), str(maxiter)] + [repr(v) for v in x0]).decode().split()
        assert words[0] == run
        out[run] = dict(iterations=int(words[1]), trial=int(words[2]), jac=int(words[3]), trace=dict(zip(TRACE, (int(w) for w in words[4:12]))),
                        x=np.array([float(w) for w in words[12:]]))
    return out


def test_dogleg_problems_are_well_conditioned():
    """The 1e-12 bound below leans on cond(J) <= 10 at the solution: ten times kappa^2 eps times a few dozen operations."""
    for pb in PROBLEMS:
        if pb.solution is not None:
            assert np.abs(pb.r(pb.solution)).max() == 0.0 and np.linalg.cond(pb.J(pb.solution)) <= 10.0, type(pb).__name__


@pytest.mark.parametrize('run', sorted(RUNS))
def test_dogleg_start_points_are_stable(run):
    """The oracle's own counts do not move when x0 moves by 1e-13 relative: the comparison below does not sit on a branch's edge."""
    _, base = _oracle(run)
    x0 = np.array(RUNS[run][3])
    for sign in (1.0, -1.0):
        _, stats = _oracle(run, x0 * (1.0 + sign * 1e-13) + sign * 1e-13 * (x0 == 0))
        assert (stats['iterations'], stats['fevals'], stats['jevals']) == (base['iterations'], base['fevals'], base['jevals'])


@pytest.mark.parametrize('run', sorted(RUNS))
def test_dogleg_matches_oracle(dogleg_runs, run):
    got = dogleg_runs[run]
    x, stats = _oracle(run)
    print(run, got['iterations'], got['trial'], got['jac'], got['trace'], np.abs(got['x'] - x).max())
    # the header evaluates once more per accepted step (residual with the Jacobian); the oracle keeps the trial residual
    assert (got['iterations'], got['trial'], got['jac']) == (stats['iterations'], stats['fevals'] - 1, stats['jevals'])
    assert np.all(np.abs(got['x'] - x) <= 1e-12 * np.maximum(1.0, np.abs(x)))
    sol = PROBLEMS[RUNS[run][0]].solution
    if sol is not None and RUNS[run][1] == 0.0:
        assert np.abs(got['x'] - sol).max() < 1e-8          # these runs converge


def test_dogleg_runs_take_every_branch(dogleg_runs):
    total = {key: sum(r['trace'][key] for r in dogleg_runs.values()) for key in TRACE}
    print(total)
    for key in ('cauchy', 'gauss_newton', 'interpolated', 'rejected', 'stop_e3', 'stop_maxiter'):
        assert total[key] > 0, key
    assert dogleg_runs['circles_e3']['trace']['stop_e3'] == 1 and dogleg_runs['powell_maxiter']['trace']['stop_maxiter'] == 1
