"""The Stage-I solver kernels of moshpp_amd/csrc/stagei.hip one by one against plain high-precision references.

tests/kernels/stagei_probe.hip includes stagei.hip unchanged and launches single kernels (or the host's kernel sequences) exactly as
moshii_stagei_core does.  Every case runs in two tiers: the CPU emulation build of the probe (no mark) and the gfx950 build (gpu mark; each
case twice, the outputs bit-identical: these kernels have fixed summation orders, so a difference is a race).

Bounds come from the operations' rounding-error analyses (u = 2^-53, gamma_k = k u / (1 - k u)); what a dropped tile, chunk, panel or
term costs is orders of magnitude above them.  Every output buffer carries NaN guard bands (and a NaN body where the kernels must write
every entry) and the guards must come back bit-identical."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.kernels import build_probe

U = 2.0 ** -53
GUARD = 64                       # stagei_probe.hip: PG
S1_NMAX, S1_FSMAX, S1_PB, S1_T, S1_NNK = 4096, 120, 32, 32, 8
SENT_F = np.array([0x7ff8_dead_beef_0001], dtype=np.uint64).view(np.float64)[0]   # a NaN with a payload no kernel produces
SENT_I = np.int32(-0x2152_4111)

TIERS = [pytest.param('emu', id='emu'), pytest.param('gpu', id='gpu', marks=pytest.mark.gpu)]


def gamma(k):
    return k * U / (1 - k * U)


@functools.lru_cache(maxsize=None)
def _lib(tier):
    lib = C.CDLL(build_probe.build(tier))
    lib.probe_gemv_t.argtypes = [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_double] + [C.c_void_p] * 2
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _buf(count, dtype=np.float64, body=None):
    """[GUARD | count | GUARD], sentinel everywhere unless `body` gives the middle."""
    b = np.full(count + 2 * GUARD, SENT_F if dtype == np.float64 else SENT_I, dtype=dtype)
    if body is not None:
        b[GUARD:GUARD + count] = np.asarray(body, dtype=dtype).ravel()
    return b


def _mid(b):
    return b[GUARD:-GUARD]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _guards_ok(b):
    ref = _buf(len(b) - 2 * GUARD, b.dtype)
    return _same_bits(b[:GUARD], ref[:GUARD]) and _same_bits(b[-GUARD:], ref[-GUARD:])


def _is_sent(a):
    return (np.ascontiguousarray(a).view(np.uint64) == np.uint64(0x7ff8_dead_beef_0001)) if a.dtype == np.float64 else (a == SENT_I)


def _run(tier, fn):
    """fn() -> dict of output arrays (guard bands included).  Guards intact; on the GPU a second run gives the same bits."""
    out = fn()
    for k, v in out.items():
        if v.dtype in (np.float64, np.int32) and len(v) > 2 * GUARD and k != 'status':
            assert _guards_ok(v), f'{k}: a guard band was written'
    if tier == 'gpu':
        again = fn()
        for k in out:
            assert _same_bits(out[k], again[k]), f'{k}: two runs of the same launch differ (race)'
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# long-double references
# ---------------------------------------------------------------------------------------------------------------------------
LD = np.longdouble


def chol_ld(A):
    """Lower Cholesky factor in long double (right-looking, vectorised updates)."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros_like(A)
    for c in range(n):
        d = np.sqrt(A[c, c])
        L[c, c] = d
        L[c + 1:, c] = A[c + 1:, c] / d
        A[c + 1:, c + 1:] -= np.outer(L[c + 1:, c], L[c + 1:, c])
    return L


def trinv_ld(L):
    """Inverse of a lower triangular matrix in long double (forward substitution on the identity)."""
    L = np.asarray(L, dtype=LD)
    n = L.shape[0]
    X = np.zeros_like(L)
    for i in range(n):
        X[i, :] = ((i == np.arange(n)).astype(LD) - L[i, :i] @ X[:i, :]) / L[i, i]
    return X


def solve_chol_ld(L, b):
    y = np.zeros(len(b), dtype=LD)
    for i in range(len(b)):
        y[i] = (LD(b[i]) - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros_like(y)
    for i in range(len(b) - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def spd(n, rng, cond=1e3):
    """Symmetric positive definite, eigenvalues log-spaced over [1 / cond, 1]: 2-norm condition number `cond`."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0, -np.log10(cond), n)) @ Q.T
    return (A + A.T) / 2


def _rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), LD(1e-300)))


# ---------------------------------------------------------------------------------------------------------------------------
# k_s1_nzflags + k_s1_syrk
# ---------------------------------------------------------------------------------------------------------------------------
def _arrow_jacobian(R, n, rng, zero_chunks=True):
    """R x n, arrow-sparse: each row chunk of 32 rows uses the columns of one 'frame' block (32 columns wide) plus the last column block
    (the 'shared' one); every fifth chunk is all zeros.  Tiles of two different frame blocks then have no used chunk at all."""
    J = np.zeros((R, n))
    ncb = (n + S1_T - 1) // S1_T
    for rc in range((R + S1_T - 1) // S1_T):
        if zero_chunks and rc % 5 == 3:
            continue
        r0, r1 = rc * S1_T, min(R, rc * S1_T + S1_T)
        fb = rc % max(1, ncb - 1)
        J[r0:r1, fb * S1_T:min(n, fb * S1_T + S1_T)] = rng.standard_normal((r1 - r0, min(n, fb * S1_T + S1_T) - fb * S1_T))
        J[r0:r1, (ncb - 1) * S1_T:] = rng.standard_normal((r1 - r0, n - (ncb - 1) * S1_T))
    return J


def _pitched(J, ldn):
    R, n = J.shape
    Jp = np.full((R, ldn), np.nan)         # NaN in the pitch padding: a kernel that reads it poisons its sums
    Jp[:, :n] = J
    return Jp


def _syrk(tier, J, ldn, given_flags=None):
    R, n = J.shape
    Jp = _pitched(J, ldn)
    nt, nrc = (n + S1_T - 1) // S1_T, (R + S1_T - 1) // S1_T

    def go():
        fl = _buf(nrc * nt, np.int32, given_flags)
        A = _buf(n * n)
        assert _lib(tier).probe_syrk(_p(Jp), R, n, ldn, int(given_flags is not None), _p(fl), _p(A)) == 0
        return dict(flags=fl, A=A)
    o = _run(tier, go)
    return _mid(o['flags']).reshape(nrc, nt), _mid(o['A']).reshape(n, n)


def _check_syrk(A, J, use=None):
    """|A - J^T J| <= 2 gamma_R |J|^T |J| elementwise (the kernel's and the float64 reference's rounding); `use` [chunk][col block]: the
    chunks a tile sums are those flagged for both of its column blocks."""
    R, n = J.shape
    assert not _is_sent(A).any() and np.isfinite(A).all(), 'an entry of A was not written'
    assert _same_bits(A, A.T), 'A is not bitwise symmetric'
    if use is None:
        ref, mag = J.T @ J, np.abs(J).T @ np.abs(J)
    else:
        ref, mag = np.zeros((n, n)), np.zeros((n, n))
        colblk = np.arange(n) // S1_T
        for rc in range(use.shape[0]):
            Jc = J[rc * S1_T:(rc + 1) * S1_T]
            m = use[rc][colblk]
            both = np.outer(m, m).astype(bool)
            ref += np.where(both, Jc.T @ Jc, 0.0)
            mag += np.where(both, np.abs(Jc).T @ np.abs(Jc), 0.0)
    err = np.abs(A - ref)
    assert (err <= 2 * gamma(R) * mag * (1 + 1e-12) + 1e-300).all(), f'SYRK error {err.max():.3e} above its bound'


SYRK_SHAPES = [(1, 1), (31, 31), (33, 32), (32768, 33), (32769, 65), (40000, 64), (31, 169), (1, 925), (600, 925), (2000, 169)]


@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('R,n', SYRK_SHAPES, ids=[f'R{r}-n{n}' for r, n in SYRK_SHAPES])
def test_syrk_normal_equations(tier, R, n):
    rng = np.random.default_rng(R * 7 + n)
    J = _arrow_jacobian(R, n, rng) if R > 1 else rng.standard_normal((R, n))
    ldn = ((n + 15) & ~15) + 16
    flags, A = _syrk(tier, J, ldn)
    ncb = (n + S1_T - 1) // S1_T
    want = np.zeros_like(flags)
    for rc in range(flags.shape[0]):
        for cb in range(ncb):
            want[rc, cb] = int((J[rc * S1_T:(rc + 1) * S1_T, cb * S1_T:(cb + 1) * S1_T] != 0).any())
    assert (flags == want).all(), 'k_s1_nzflags'
    _check_syrk(A, J)


@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('R,n', [(32768, 96), (40000, 96), (1200, 169)])
def test_syrk_sums_exactly_the_flagged_chunks(tier, R, n):
    """k_s1_syrk's contract with its flags: a tile sums the row chunks flagged for BOTH of its column blocks -- below and beyond the
    S1_SYRK_CHUNKS chunks whose flags it caches in LDS.  Dense J, flags that leave chunks out per column block."""
    rng = np.random.default_rng(n)
    J = rng.standard_normal((R, n))
    nrc, ncb = (R + S1_T - 1) // S1_T, (n + S1_T - 1) // S1_T
    use = (rng.random((nrc, ncb)) < 0.6).astype(np.int32)
    _, A = _syrk(tier, J, n + 16, given_flags=use)
    _check_syrk(A, J, use)


@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('F,fs,ns', [(6, 17, 96), (12, 69, 169), (1, 3, 1)])
def test_syrk_all_ones_flags_on_y(tier, F, fs, ns):
    """The Schur path's form: T = Y^T Y over F fs rows of pitch nsp = ns rounded up to 16, all-ones flags."""
    rng = np.random.default_rng(fs)
    Y = rng.standard_normal((F * fs, ns))
    nsp = (ns + 15) & ~15
    ones = np.ones(((F * fs + S1_T - 1) // S1_T, (ns + S1_T - 1) // S1_T), np.int32)
    _, T = _syrk(tier, Y, nsp, given_flags=ones)
    _check_syrk(T, Y)


# ---------------------------------------------------------------------------------------------------------------------------
# k_s1_gemv_t + k_s1_gemv_t_sum, k_s1_gemv
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('R,n,sign', [(1, 1, -1.0), (5, 300, 1.0), (15, 257, -1.0), (1001, 925, -1.0), (4099, 33, 1.0)])
def test_gemv_t(tier, R, n, sign):
    rng = np.random.default_rng(R + n)
    J, r = rng.standard_normal((R, n)), rng.standard_normal(R)
    ldn = ((n + 15) & ~15) + 16
    Jp = _pitched(J, ldn)

    def go():
        part, y = _buf(16 * n), _buf(n)
        assert _lib(tier).probe_gemv_t(_p(Jp), _p(r), R, n, ldn, sign, _p(part), _p(y)) == 0
        return dict(part=part, y=y)
    o = _run(tier, go)
    y, part = _mid(o['y']), _mid(o['part']).reshape(16, n)
    per = (R + 15) // 16
    for c in range(16):     # chunk c holds rows [c per, (c + 1) per) of R; an empty chunk sums to an exact 0
        rows = slice(min(R, c * per), min(R, (c + 1) * per))
        ref = J[rows].T @ r[rows]
        assert (np.abs(part[c] - ref) <= 2 * gamma(per) * (np.abs(J[rows]).T @ np.abs(r[rows])) + 1e-300).all(), c
        if rows.start == rows.stop:
            assert (part[c] == 0).all()
    ref = sign * (J.T.astype(LD) @ r.astype(LD))
    assert (np.abs(y - ref) <= gamma(R + 16) * (np.abs(J).T @ np.abs(r)) + 1e-300).all()


@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('rows,n,ld', [(1, 1, 1), (31, 31, 47), (300, 300, 300), (925, 925, 941), (5, 4096, 4096)])
def test_gemv(tier, rows, n, ld):
    rng = np.random.default_rng(n)
    M, x = rng.standard_normal((rows, n)), rng.standard_normal(n)
    Mp = np.full((rows, ld), np.nan)
    Mp[:, :n] = M

    def go():
        y = _buf(rows)
        assert _lib(tier).probe_gemv(_p(Mp), _p(x), rows, n, ld, _p(y)) == 0
        return dict(y=y)
    y = _mid(_run(tier, go)['y'])
    ref = M.astype(LD) @ x.astype(LD)
    assert (np.abs(y - ref) <= gamma(n) * (np.abs(M) @ np.abs(x)) + 1e-300).all()


# ---------------------------------------------------------------------------------------------------------------------------
# blocked Cholesky (k_s1_chol_diag / _trsm / _update, panel by panel as the host loops) + k_s1_tri_solve
# ---------------------------------------------------------------------------------------------------------------------------
def _chol(tier, A, g):
    n = A.shape[0]
    nd = (n + S1_PB - 1) // S1_PB * S1_PB * S1_PB

    def go():
        Ab, D, x = _buf(n * n, body=A), _buf(nd), _buf(n)
        st = np.zeros(3, np.int32)
        assert _lib(tier).probe_chol(_p(Ab), n, _p(D), _p(g), _p(x), _p(st)) == 0
        return dict(A=Ab, dinv=D, x=x, status=st)
    o = _run(tier, go)
    return (_mid(o['A']).reshape(n, n), _mid(o['dinv']).reshape(-1, S1_PB, S1_PB), _mid(o['x']), o['status'])


def _kappa_inf(L, Li):
    return float(np.abs(L).sum(1).max() * np.abs(Li).sum(1).max())


CHOL_N = [1, 2, 31, 32, 33, 63, 64, 65, 96, 114, 169, 925, 4096]


@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('n', CHOL_N)
def test_blocked_cholesky_and_tri_solve(tier, n):
    rng = np.random.default_rng(n)
    cond = 1e3
    A = spd(n, rng, cond)
    g = rng.standard_normal(n)
    F, D, x, st = _chol(tier, A, g)
    assert st[1] == 0 and st[0] == 0 and st[2] == 0
    iu = np.triu_indices(n, 1)
    assert _same_bits(F[iu], A[iu]), 'the strict upper triangle was written'
    L = np.tril(F)
    assert np.isfinite(L).all()
    # dinv: panel p holds L_D^-1 of its diagonal block (the tail panel's block: jb x jb); backward-style bound of a triangular inverse
    kD = 1.0
    for p in range((n + S1_PB - 1) // S1_PB):
        j0 = p * S1_PB
        jb = min(S1_PB, n - j0)
        LD_ = L[j0:j0 + jb, j0:j0 + jb]
        Xref = trinv_ld(LD_)
        kD = max(kD, _kappa_inf(LD_, Xref))
        got = D[p, :jb, :jb]
        assert (np.triu(got, 1) == 0).all()
        # |X - L^-1| <= c_n |L^-1| |L| |X| (Higham, Thm 14.? for substitution-based inverses), c_n = gamma_jb
        bound = gamma(jb) * (np.abs(Xref) @ np.abs(LD_) @ np.abs(got)).astype(float)
        assert (np.abs(got - Xref) <= 2 * bound + 1e-300).all(), f'dinv of panel {p}'
    # backward error of the factor: A = L L^T + dA with |dA| <= gamma_{n+1} (1 + max_D kappa(L_D)) |L||L^T| (the blocked algorithm applies
    # each panel through its diagonal block's computed inverse), plus gamma_n of the float64 product that checks it
    LLt = L @ L.T
    mag = np.abs(L) @ np.abs(L).T
    bound = (gamma(n + 1) * (1 + kD) + gamma(n)) * mag
    err = np.abs(np.tril(A - LLt))
    assert (err <= np.tril(bound) + 1e-300).all(), f'backward error {(err / np.maximum(mag, 1e-300)).max():.3e}'
    # against the reference factor and solution: first-order perturbation bounds, kappa_2(A) = cond
    if n <= 925:
        Lr = chol_ld(A)
        xr = solve_chol_ld(Lr, g)
    else:
        Lr = np.linalg.cholesky(A)
        xr = np.linalg.solve(A, g)
    tol = 4 * cond * (n + 1) * U * (1 + kD)
    assert _rel(L, Lr) <= tol, f'factor {_rel(L, Lr):.3e} vs {tol:.3e}'
    assert _rel(x, xr) <= tol, f'solution {_rel(x, xr):.3e} vs {tol:.3e}'


@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('kind', ['zero', 'negative', 'nan'])
@pytest.mark.parametrize('where', ['first', 'middle', 'tail'])
def test_cholesky_non_positive_pivot_sets_status(tier, kind, where):
    """A zero, negative or NaN pivot in the first panel, a middle panel or the tail panel raises status[1].  The pivot's row and column
    are zero elsewhere, so the zero pivot is exactly zero at its step."""
    n = 100                                         # panels [0, 32) [32, 64) [64, 96) [96, 100)
    k = {'first': 5, 'middle': 40, 'tail': 97}[where]
    rng = np.random.default_rng(k)
    A = spd(n, rng, 1e2)
    A[k, :] = 0.0
    A[:, k] = 0.0
    A[k, k] = {'zero': 0.0, 'negative': -1.0, 'nan': np.nan}[kind]
    _, _, _, st = _chol(tier, A, rng.standard_normal(n))
    assert st[1] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# the arrow-structured step: k_s1_elim, k_s1_elim_y, SYRK on Y, k_s1_schur_sub, Cholesky on S, k_s1_tri_solve, k_s1_back
# ---------------------------------------------------------------------------------------------------------------------------
def _arrow_system(F, fs, ns, rng, cond=1e2):
    """Full symmetric A (n = F fs + ns) with arrow structure: frame blocks A_ff (SPD, condition `cond`), couplings A_fs, and
    A_ss = sum_f A_fs^T A_ff^-1 A_fs + S0 with S0 SPD (condition `cond`): the Schur complement of all frames is S0.  Frame and
    shared columns are spread over [0, n) by a random permutation."""
    n = F * fs + ns
    perm = rng.permutation(n)
    fcols = perm[:F * fs].reshape(F, fs).astype(np.int32)
    scols = perm[F * fs:].astype(np.int32)
    A = np.zeros((n, n))
    Ass = spd(ns, rng, cond) * 4.0
    for f in range(F):
        Aff = spd(fs, rng, cond) * 2.0
        Afs = rng.standard_normal((fs, ns)) * 0.3
        A[np.ix_(fcols[f], fcols[f])] = Aff
        A[np.ix_(fcols[f], scols)] = Afs
        A[np.ix_(scols, fcols[f])] = Afs.T
        Ass += Afs.T @ np.linalg.solve(Aff, Afs)
    A[np.ix_(scols, scols)] = (Ass + Ass.T) / 2
    return A, fcols, scols


def _schur(tier, A, g, fcols, scols, fbase=0, nown=None, scatter=1):
    F, fs = fcols.shape
    ns, n = len(scols), A.shape[0]
    nown = F - fbase if nown is None else nown
    nsp = (ns + 15) & ~15
    nd = (ns + S1_PB - 1) // S1_PB * S1_PB * S1_PB

    def go():
        b = dict(Linv=_buf(F * fs * fs), Y=_buf(F * fs * nsp), z=_buf(F * fs), T=_buf(ns * ns), S=_buf(ns * ns), h=_buf(ns),
                 dinv=_buf(nd), ds=_buf(ns), out=_buf(n), status=np.zeros(3, np.int32))
        assert _lib(tier).probe_schur(_p(A), n, _p(g), _p(fcols), F, fs, _p(scols), ns, fbase, nown, scatter,
                                      *[_p(b[k]) for k in ('Linv', 'Y', 'z', 'T', 'S', 'h', 'dinv', 'ds', 'out', 'status')]) == 0
        return b
    o = _run(tier, go)
    r = {k: _mid(v) for k, v in o.items() if k != 'status'}
    r['status'] = o['status']
    r['Linv'] = r['Linv'].reshape(F, fs, fs)
    r['Y'] = r['Y'].reshape(F, fs, nsp)
    r['z'] = r['z'].reshape(F, fs)
    r['T'] = r['T'].reshape(ns, ns)
    r['S'] = r['S'].reshape(ns, ns)
    return r


def _schur_reference(A, g, fcols, scols, frames):
    """The same elimination in long double, over the frames `frames`: L_f^-1, Y_f, z_f, S, h, d_s and every frame's d_f."""
    Al, gl = A.astype(LD), g.astype(LD)
    Ass = Al[np.ix_(scols, scols)]
    ref = dict(Linv={}, Y={}, z={}, d={})
    S, h = Ass.copy(), gl[scols].copy()
    for f in frames:
        Li = trinv_ld(chol_ld(Al[np.ix_(fcols[f], fcols[f])]))
        Y = Li @ Al[np.ix_(fcols[f], scols)]
        z = Li @ gl[fcols[f]]
        ref['Linv'][f], ref['Y'][f], ref['z'][f] = Li, Y, z
        S -= Y.T @ Y
        h -= Y.T @ z
    ref['S'], ref['h'], ref['T'] = S, h, Ass - S
    ref['ds'] = solve_chol_ld(chol_ld(S), h)
    for f in frames:
        ref['d'][f] = ref['Linv'][f].T @ (ref['z'][f] - ref['Y'][f] @ ref['ds'])
    return ref


SCHUR_CASES = [(1, 1, 1), (6, 3, 31), (6, 17, 32), (12, 69, 33), (6, 93, 96), (12, 117, 169), (12, 120, 169), (1, 120, 1), (6, 120, 33),
               (12, 3, 169)]


@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('F,fs,ns', SCHUR_CASES, ids=[f'F{a}-fs{b}-ns{c}' for a, b, c in SCHUR_CASES])
def test_schur_step(tier, F, fs, ns):
    rng = np.random.default_rng(F * 1000 + fs * 10 + ns)
    cond = 1e2
    A, fcols, scols = _arrow_system(F, fs, ns, rng, cond)
    n = A.shape[0]
    g = rng.standard_normal(n)
    o = _schur(tier, A, g, fcols, scols)
    assert (o['status'] == 0).all()
    ref = _schur_reference(A, g, fcols, scols, range(F))
    # every intermediate within a first-order bound: c kappa (size) u with kappa the (2-norm) condition numbers of the blocks (cond),
    # of the whole system (<= cond^2 here) for what depends on all of it
    tf = 8 * cond * (fs + 1) * U
    ts = 8 * cond ** 2 * (n + 1) * U
    for f in range(F):
        assert _rel(np.tril(o['Linv'][f]), ref['Linv'][f]) <= tf, f'Linv frame {f}'
        assert (np.triu(o['Linv'][f], 1) == 0).all()
        assert _rel(o['Y'][f][:, :ns], ref['Y'][f]) <= tf, f'Y frame {f}'
        assert (o['Y'][f][:, ns:] == 0).all(), 'Y pitch padding written'
        assert _rel(o['z'][f], ref['z'][f]) <= tf, f'z frame {f}'
    S_lo = np.tril(o['S'])
    assert _rel(o['h'], ref['h']) <= ts
    assert _rel(o['T'], ref['T']) <= ts
    # S went through the Cholesky in place: its lower triangle is the factor of A_ss - T
    assert _rel(S_lo @ S_lo.T, ref['S']) <= ts
    assert _rel(o['ds'], ref['ds']) <= ts
    step = o['out']
    assert not _is_sent(step).any(), 'an unknown of the step was not written'
    d_ref = np.zeros(n, dtype=LD)
    d_ref[scols] = ref['ds']
    for f in range(F):
        d_ref[fcols[f]] = ref['d'][f]
    assert _rel(step, d_ref) <= ts
    # and as a solve of the whole system: the residual of the step, relative to |A||d| + |g|
    res = np.abs(A.astype(LD) @ step.astype(LD) - g)
    assert float(res.max() / (np.abs(A) @ np.abs(step) + np.abs(g)).max()) <= ts


@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('scatter', [0, 1])
def test_schur_step_sharded(tier, scatter):
    """One rank's share: frames [fbase, fbase + nown) of F (fbase != 0).  S and h hold only those frames' contributions, k_s1_back writes
    only their columns (and the shared ones when scatter_shared = 1); the other frames' factors stay unwritten."""
    F, fs, ns, fbase, nown = 12, 17, 96, 4, 5
    rng = np.random.default_rng(11)
    A, fcols, scols = _arrow_system(F, fs, ns, rng)
    n = A.shape[0]
    g = rng.standard_normal(n)
    o = _schur(tier, A, g, fcols, scols, fbase, nown, scatter)
    assert (o['status'] == 0).all()
    own = range(fbase, fbase + nown)
    ref = _schur_reference(A, g, fcols, scols, own)
    ts = 8 * 1e4 * (n + 1) * U
    for f in range(F):
        if f in own:
            assert _rel(o['Y'][f][:, :ns], ref['Y'][f]) <= 1e-11 and not _is_sent(o['Linv'][f]).any()
        else:
            assert _is_sent(o['Linv'][f]).all() and (o['Y'][f] == 0).all() and (o['z'][f] == 0).all()
    assert _rel(o['h'], ref['h']) <= ts and _rel(o['ds'], ref['ds']) <= ts
    step = o['out']
    written = ~_is_sent(step)
    want = np.zeros(n, bool)
    for f in own:
        want[fcols[f]] = True
    if scatter:
        want[scols] = True
    assert (written == want).all(), 'k_s1_back wrote columns it does not own (or missed its own)'
    for f in own:
        assert _rel(step[fcols[f]], ref['d'][f]) <= ts
    if scatter:
        assert _rel(step[scols], ref['ds']) <= ts


@pytest.mark.parametrize('tier', TIERS)
def test_schur_non_positive_pivot_in_a_frame_block(tier):
    F, fs, ns = 6, 17, 33
    rng = np.random.default_rng(5)
    A, fcols, scols = _arrow_system(F, fs, ns, rng)
    k = fcols[3, 9]
    A[k, :] = 0.0
    A[:, k] = 0.0
    A[k, k] = -2.0
    o = _schur(tier, A, rng.standard_normal(A.shape[0]), fcols, scols)
    assert o['status'][1] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# k_s1_knn + k_s1_pick3
# ---------------------------------------------------------------------------------------------------------------------------
def _knn(tier, can, excl, ml):
    V, M = len(can), len(ml)

    def go():
        c8, c3 = _buf(S1_NNK * M, np.int32), _buf(3 * M, np.int32)
        st = np.zeros(3, np.int32)
        assert _lib(tier).probe_knn(_p(np.ascontiguousarray(can)), _p(np.ascontiguousarray(excl, dtype=np.uint8)), V,
                                    _p(np.ascontiguousarray(ml)), M, _p(c8), _p(c3), _p(st)) == 0
        return dict(cl8=c8, cl=c3, status=st)
    o = _run(tier, go)
    return _mid(o['cl8']).reshape(M, S1_NNK), _mid(o['cl']).reshape(M, 3), o['status']


def _knn_reference(can, excl, ml):
    ids = np.flatnonzero(~excl.astype(bool))
    out = []
    for x in ml:
        d2 = ((x - can[ids]) ** 2).sum(1)         # exact on the dyadic lattice
        out.append(ids[np.lexsort((ids, d2))[:S1_NNK]])
    return np.array(out, dtype=np.int32)


def _pick3_reference(can, c8):
    M = len(c8)
    nn = 3
    while True:
        e1 = can[c8[:, 1]] - can[c8[:, 0]]
        e2 = can[c8[:, nn - 1]] - can[c8[:, 0]]
        cr = np.cross(e1, e2)
        bad = bool(((cr * cr).sum(1) == 0).any())
        if not bad or nn >= S1_NNK or nn >= M:
            return np.stack([c8[:, 0], c8[:, 1], c8[:, nn - 1]], 1), nn, bad
        nn += 1


def _lattice(V, rng, side=4, step=0.25):
    """Dyadic lattice points (many exact duplicates and equal distances)."""
    return (rng.integers(0, side, size=(V, 3)) * step).astype(np.float64)


@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('V', [8, 255, 256, 257, 6890])
def test_knn_exact_ties_and_pick3(tier, V):
    rng = np.random.default_rng(V)
    can = _lattice(V, rng, side=3 if V < 300 else 6)
    excl = np.zeros(V, np.uint8)
    if V > 8:
        excl[rng.choice(V, V // 5, replace=False)] = 1
    M = 40
    ml = (rng.integers(-2, 14, size=(M, 3)) * 0.125).astype(np.float64)
    c8, cl, st = _knn(tier, can, excl, ml)
    want = _knn_reference(can, excl, ml)
    assert (c8 == want).all(), 'nearest 8: (distance, lower id first) order'
    w3, _, bad = _pick3_reference(can, want)
    assert (cl == w3).all()
    assert st[2] == int(bad)


@pytest.mark.parametrize('tier', TIERS)
def test_pick3_collinear_triple_moves_every_marker_on(tier):
    """Marker 0's three nearest vertices lie on one line: the third neighbour of EVERY marker moves to its fourth nearest."""
    rng = np.random.default_rng(3)
    V, M = 300, 20
    can = _lattice(V, rng, side=4096, step=2.0 ** -8) + 4.0     # a cloud in general position away from the origin (exact in binary)
    can[:4] = [[0, 0, 0], [0.5, 0, 0], [-1.0, 0, 0], [0, 1.5, 0]]
    ml = np.vstack([[[0.125, 0, 0]], can[4:M + 3] + 2.0 ** -10])
    excl = np.zeros(V, np.uint8)
    c8, cl, st = _knn(tier, can, excl, ml)
    want = _knn_reference(can, excl, ml)
    assert (c8 == want).all()
    assert list(want[0, :4]) == [0, 1, 2, 3]
    w3, nn, bad = _pick3_reference(can, want)
    assert nn == 4 and not bad
    assert (cl == w3).all() and (cl[:, 2] == want[:, 3]).all()
    assert st[2] == 0


@pytest.mark.parametrize('tier', TIERS)
def test_pick3_all_collinear_raises_status(tier):
    V, M = 64, 5
    can = np.zeros((V, 3))
    can[:, 0] = np.arange(V) * 0.5
    ml = np.array([[1.25, 0.5, 0.0], [10.0, 0.25, 0.25], [3.0, -1.0, 0.0], [20.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    excl = np.zeros(V, np.uint8)
    c8, cl, st = _knn(tier, can, excl, ml)
    want = _knn_reference(can, excl, ml)
    assert (c8 == want).all()
    w3, nn, bad = _pick3_reference(can, want)
    assert bad and nn == min(S1_NNK, M)
    assert (cl == w3).all() and st[2] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# k_s1_surface
# ---------------------------------------------------------------------------------------------------------------------------
def _octahedron(levels, rng):
    """Closed octahedron |x| + |y| + |z| = 1, every face split into 4^levels coplanar ones (dyadic midpoints), faces shuffled."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                a, b, c = v.index((sx, 0, 0)), v.index((0, sy, 0)), v.index((0, 0, sz))
                f.append((a, b, c) if sx * sy * sz > 0 else (a, c, b))       # outward normals
    verts = [np.array(p, dtype=np.float64) for p in v]
    key = {tuple(p): i for i, p in enumerate(v)}

    def mid(i, j):
        p = (verts[i] + verts[j]) / 2
        t = tuple(p)
        if t not in key:
            key[t] = len(verts)
            verts.append(p)
        return key[t]
    for _ in range(levels):
        nf = []
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    f = np.array(f, dtype=np.int32)[rng.permutation(len(f))]
    return np.array(verts), np.ascontiguousarray(f)


def _surface(tier, can, faces, ml):
    V, nf, M = len(can), len(faces), len(ml)
    cnt = np.bincount(faces.ravel(), minlength=V)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    lst = np.zeros(3 * nf, np.int32)
    fill = ptr[:-1].copy()
    for fi in range(nf):
        for c in range(3):
            lst[fill[faces[fi, c]]] = fi
            fill[faces[fi, c]] += 1

    def go():
        b = dict(sdist=_buf(M), tv=_buf(3 * M, np.int32), sdp=_buf(3 * M), sdabc=_buf(9 * M))
        assert _lib(tier).probe_surface(_p(can), V, _p(faces), nf, _p(ptr), _p(lst), _p(np.ascontiguousarray(ml)), M,
                                        _p(b['sdist']), _p(b['tv']), _p(b['sdp']), _p(b['sdabc'])) == 0
        return b
    o = _run(tier, go)
    return _mid(o['sdist']), _mid(o['tv']).reshape(M, 3), _mid(o['sdp']).reshape(M, 3), _mid(o['sdabc']).reshape(M, 3, 3)


def _per_vertex(V, fv, dabc):
    g = np.zeros((len(fv), V, 3))
    for m in range(len(fv)):
        for s in range(3):
            g[m, fv[m, s]] += dabc[m, s]
    return g


@pytest.mark.parametrize('tier', TIERS)
@pytest.mark.parametrize('levels', [1, 4])
def test_surface_against_oracle(tier, levels):
    """levels 1: 32 faces (fewer than the 1024 threads), 4: 2048 faces (two a thread, all 16 waves in the arg-min)."""
    from oracle import stagei_oracle as s1
    rng = np.random.default_rng(levels)
    can, faces = _octahedron(levels, rng)
    V = len(can)
    s_ = np.sign(can)
    corners = [i for i in range(V) if np.abs(can[i]).max() == 1.0]
    flat = [i for i in range(V) if (can[i] != 0).all()][:24]          # inside one octant's face: 6 coplanar faces around it
    # exact ties: out of the 6 corners (4 faces each), and along the normal of flat vertices from outside and from inside (6 faces each).
    # Dyadic coordinates and offsets: every face's closest point is the vertex itself, bit for bit, fused multiply-adds or not
    P_vert = np.vstack([can[corners] * 1.5, can[flat] + 0.25 * s_[flat], can[flat] - 0.0625 * s_[flat]])
    # shared edges (the winner's choice may depend on rounding): midpoints pushed out along the corner direction
    e = faces[:24]
    P_edge = np.vstack([(can[a] + can[b]) / 2 * 1.25 for a, b, _ in e])
    # face interiors: along the face normal from the centroid, outside and inside (one face each)
    ctr = can[faces[24:48]].mean(1)
    P_face = np.vstack([ctr + 0.125 * np.sign(ctr), ctr - 0.03125 * np.sign(ctr)])
    ml = np.vstack([P_vert, P_edge, P_face])
    sd, tv, dp, dabc = _surface(tier, can, faces, ml)
    rd, rtri, rpart, rdp, rdabc, rfv = s1.signed_surface_distance(ml, can, faces, want_jac=True)
    nv = len(P_vert)
    exact = np.r_[np.arange(nv), np.arange(nv + len(P_edge), len(ml))]
    # distance ties broken the same way: lowest face id, all quantities
    assert (tv[exact] == rfv[exact]).all(), 'nearest face (lowest id on exact ties)'
    assert np.abs(sd - rd).max() <= 1e-14
    assert np.abs(dp - rdp).max() <= 1e-12
    assert np.abs(dabc[exact] - rdabc[exact]).max() <= 1e-12
    # every marker: the gradient summed per vertex id does not depend on which face won
    assert np.abs(_per_vertex(V, tv, dabc) - _per_vertex(V, rfv, rdabc)).max() <= 1e-12
    assert ((sd < 0) == (np.abs(ml).sum(1) < 1)).all(), 'sign: inside vs outside'
    # central differences of the signed distance (markers off the ties: the face interiors and edges)
    h = 1e-6
    for m in list(range(nv, len(ml)))[::6]:
        for a in range(3):
            xp, xm = ml[m].copy(), ml[m].copy()
            xp[a] += h
            xm[a] -= h
            fd = (s1.signed_surface_distance(xp[None], can, faces)[0][0] - s1.signed_surface_distance(xm[None], can, faces)[0][0]) / (2 * h)
            assert abs(fd - dp[m, a]) <= 1e-6
        gv = _per_vertex(V, tv[m:m + 1], dabc[m:m + 1])[0]
        for vid in set(tv[m]):
            for a in range(3):
                cp, cm = can.copy(), can.copy()
                cp[vid, a] += h
                cm[vid, a] -= h
                fd = (s1.signed_surface_distance(ml[m:m + 1], cp, faces)[0][0] - s1.signed_surface_distance(ml[m:m + 1], cm, faces)[0][0]) / (2 * h)
                assert abs(fd - gv[vid, a]) <= 1e-6
