"""The NCut eigensolver (usc_ncut_fiedler_ex, ncut.hip) on every launch plan it has, against float64 references.

The solver restates LAPACK dsygvx('L') for (D - W) x = lambda D x: Householder tridiagonalisation (stepwise or one of
four one-launch forms), Sturm bisection with inverse iteration (LDS or global work arrays), back-transformation (four
kernels).  Which of them runs depends on S (usc_ncut_fiedler_plan); the sizes below reach every plan code of this
device, the boundaries between them, sizes where most one-launch workgroups leave their last row slot empty (rows go
round-robin over G = 64 workgroups: at 129 and 130, R = 3 and only workgroup 0, or 0 and 1, fill slot 2), and the
stepwise-only range above 4000.

Graph families (Abin u8[S,S] and deg f64[S] on the device; references in float64 on the CPU):
  P  a path with its nodes relabelled, eps = 0: lambda_k = 2 sin^2(pi k / (2 (S-1))), x_j ~ cos(pi k j / (S-1))
  C  a planted two-cluster graph with the product's eps = 1e-5 and deg = full row sums: scipy's dsygvx
  X  the product's painted form: deg from the unpainted graph, ~30 % of the rows and columns of Abin cleared, the
     upper triangle random bits (only the lower triangle is read: uplo = 'L')
With y = D^1/2 x and C = D^-1/2 (D - W) D^-1/2 (||C|| <= 2), tol = 64 n eps:
  |lambda - lambda_ref| <= tol, | ||y|| - 1 | <= tol, ||C y - lambda y|| <= tol, sin(y, y_ref) <= tol / gap where
  tol / gap < 1e-2, and on C the sign of scipy's vector."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS64 = 2.2e-16
SIZES = [3, 4, 5, 7, 8, 9, 15, 17, 127, 128, 129, 130, 511, 512, 513, 640, 641, 768, 769, 800, 801, 1024, 1025, 2500,
         4000, 4001, 6000, 8000]
CASES = [(fam, S) for S in SIZES for fam in "PCX" if not (fam == "C" and S < 16)]


def _cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def _path(S, rng):
    perm = rng.permutation(S)                  # node perm[j] sits at position j of the path
    A = np.zeros((S, S), dtype=bool)
    A[perm[:-1], perm[1:]] = True
    A[perm[1:], perm[:-1]] = True
    deg = A.sum(1).astype(np.float64)
    k = np.arange(3)
    lam = 2.0 * np.sin(np.pi * k / (2.0 * (S - 1))) ** 2
    x = np.empty(S)
    x[perm] = np.cos(np.pi * np.arange(S) / (S - 1))
    y = np.sqrt(deg) * x
    return A, deg, 0.0, lam, y / np.linalg.norm(y)


def _planted(S, rng, p_in=0.3, p_out=0.01):
    side = rng.permutation(S) < S // 2
    prob = np.where(side[:, None] == side[None, :], p_in, p_out)
    A = np.triu(rng.random((S, S)) < prob, 1)
    return A | A.T


def _laplacian(A, deg, eps):
    W = np.where(A, 1.0, eps)
    L = -W
    L[np.diag_indices_from(L)] += deg
    return L


def _case(fam, S):
    """-> (Abin as the device gets it, deg, eps, reference (lambda_1, lambda_2, lambda_3), y_ref, lower-triangle A)."""
    import scipy.linalg

    rng = np.random.default_rng(7919 * S + "PCX".index(fam))
    if fam == "P":
        A, deg, eps, lam, y = _path(S, rng)
        return A.astype(np.uint8), deg, eps, lam, y, A
    eps = 1e-5
    A = _planted(S, rng)
    deg = np.where(A, 1.0, eps).sum(1)         # full row sums, diagonal (eps) included: ncut_degree_kernel
    if fam == "C":
        w, v = scipy.linalg.eigh(_laplacian(A, deg, eps), np.diag(deg), subset_by_index=[1, 2], driver="gvx")
        assert (w[1] - w[0]) / w[1] >= 0.2, w  # well separated: the vector and its sign are well defined
        y = np.sqrt(deg) * v[:, 0]
        return A.astype(np.uint8), deg, eps, np.array([0.0, w[0], w[1]]), y, A
    painted = rng.random(S) < 0.3               # X: painted after the degree, as ncut_binarize_kernel does
    A[painted, :] = False
    A[:, painted] = False
    low = np.tril(A)
    Abin = low.astype(np.uint8)
    iu = np.triu_indices(S, 1)
    Abin[iu] = rng.integers(0, 2, size=len(iu[0]), dtype=np.uint8)   # garbage the solver must not read
    sq = np.sqrt(deg)
    Cm = _laplacian(low | low.T, deg, eps) / sq[:, None] / sq[None, :]
    w, v = scipy.linalg.eigh(Cm, subset_by_index=[0, 2])
    return Abin, deg, eps, w, v[:, 1], low | low.T


def _solve(ncut, Ab, db, eps, stepwise=False):
    evec, evals = ncut._fiedler(Ab, db, eps, stepwise=stepwise)
    return evec.cpu().numpy(), evals.cpu().numpy(), evec, evals


def _sin(y, r):
    y = y / np.linalg.norm(y)
    r = r / np.linalg.norm(r)
    return float(np.linalg.norm(y - (y @ r) * r))


@pytest.mark.parametrize("fam,S", CASES, ids=[f"{f}{S}" for f, S in CASES])
def test_fiedler_matches_float64_reference(device, fam, S):
    from unscene3d_amd._lib import lib
    from unscene3d_amd.pseudo_masks import ncut

    Abin, deg, eps, lam, y_ref, A = _case(fam, S)
    Ab = torch.from_numpy(Abin).to(device)
    db = torch.from_numpy(deg).to(device)
    x, ev, evec, evals = _solve(ncut, Ab, db, eps)
    plan = lib.usc_ncut_fiedler_plan(S, _cus(device), 0)
    assert np.isfinite(x).all() and np.isfinite(ev).all(), hex(plan)
    tol = 64 * S * EPS64
    assert abs(ev[0] - lam[1]) <= tol and abs(ev[1] - lam[2]) <= tol, (hex(plan), ev, lam[1:])
    sq = np.sqrt(deg)
    y = sq * x
    assert abs(np.linalg.norm(y) - 1.0) <= tol, (hex(plan), np.linalg.norm(y) - 1.0)
    Cy = (_laplacian(A, deg, eps) @ x) / sq
    res = float(np.linalg.norm(Cy - ev[0] * y))
    assert res <= tol, (hex(plan), res, tol)
    gap = min(lam[1] - lam[0], lam[2] - lam[1])
    if tol < 1e-2 * gap:                       # (a zero gap on small painted graphs: no angle to check)
        assert _sin(y, y_ref) <= tol / gap, (hex(plan), _sin(y, y_ref), tol / gap)
    if fam == "C":
        assert float(y @ y_ref) > 0, hex(plan)     # scipy's sign (undefined on painted graphs)
    # bit-reproducible; the one-launch forms and the stepwise path round alike
    x2, ev2, _, _ = _solve(ncut, Ab, db, eps)
    assert np.array_equal(x, x2) and np.array_equal(ev, ev2), hex(plan)
    if 8 <= S <= 4000:
        assert plan & 0xF != 0 or _cus(device) < 8, hex(plan)
        _, _, evec_s, evals_s = _solve(ncut, Ab, db, eps, stepwise=True)
        assert torch.equal(evec, evec_s) and torch.equal(evals, evals_s), hex(plan)


def test_sweep_reaches_every_plan_code(device):
    from unscene3d_amd._lib import lib

    cus = _cus(device)
    reachable = {lib.usc_ncut_fiedler_plan(S, cus, 0) for S in range(3, 8001)}
    swept = {lib.usc_ncut_fiedler_plan(S, cus, 0) for S in SIZES}
    print(f"{cus} CUs, plan codes reached:", sorted(hex(c) for c in swept))
    assert swept == reachable, sorted(hex(c) for c in reachable - swept)
    assert {S for fam, S in CASES if fam == "C"} >= {S for S in SIZES if S >= 16}


def test_bad_arguments_fail_before_any_launch(device):
    from unscene3d_amd import _lib, ops
    from unscene3d_amd.pseudo_masks import ncut

    A2 = torch.ones((2, 2), dtype=torch.uint8, device=device)
    with pytest.raises(RuntimeError, match="3 <= S <= 8000"):
        ncut._fiedler(A2, torch.ones(2, dtype=torch.float64, device=device), 1e-5)
    buf = torch.zeros(64, dtype=torch.float64, device=device)
    p = buf.data_ptr()
    rc = _lib.lib.usc_ncut_fiedler_ex(p, p, 8001, 1e-5, p, p, p, 64 * 8, ops._stream(), 0)   # the workspace is short too
    assert rc != 0 and "3 <= S <= 8000" in _lib.last_error()
    S = 100
    need = _lib.lib.usc_ncut_fiedler_ws_bytes(S)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    A = torch.ones((S, S), dtype=torch.uint8, device=device)
    d = torch.full((S,), float(S), dtype=torch.float64, device=device)
    out = torch.zeros(S, dtype=torch.float64, device=device)
    for flags in (0, 1):
        rc = _lib.lib.usc_ncut_fiedler_ex(A.data_ptr(), d.data_ptr(), S, 1e-5, out.data_ptr(), out.data_ptr(),
                                          ws.data_ptr(), need - 1, ops._stream(), flags)
        assert rc != 0 and "workspace too small" in _lib.last_error()
    torch.cuda.synchronize()
    assert not out.any()                            # nothing ran


class _NaNFirst:
    """Wraps ncut._fiedler: the output of the first `bad` one-launch solves is overwritten with NaN (after the solver
    ran on finite inputs), as a solve that gave up at the spin limit would leave it."""

    def __init__(self, real, bad):
        self.real, self.bad, self.calls = real, bad, []

    def __call__(self, A, D, eps, stepwise=False):
        evec, evals = self.real(A, D, eps, stepwise=stepwise)
        self.calls.append(stepwise)
        if len(self.calls) <= self.bad:
            evec.fill_(float("nan"))
            evals.fill_(float("nan"))
        return evec, evals


def test_non_finite_eigenvector_is_solved_again_stepwise(device, monkeypatch):
    from unscene3d_amd.pseudo_masks import ncut

    Abin, deg, eps, lam, y_ref, _ = _case("C", 130)
    Ab, db = torch.from_numpy(Abin).to(device), torch.from_numpy(deg).to(device)
    _, clean = ncut.second_smallest_eigenvector(Ab, db, eps)
    wrap = _NaNFirst(ncut._fiedler, bad=1)
    monkeypatch.setattr(ncut, "_fiedler", wrap)
    with pytest.warns(RuntimeWarning, match="stepwise"):
        _, vec = ncut.second_smallest_eigenvector(Ab, db, eps)
    assert wrap.calls == [False, True]
    assert np.array_equal(vec, clean)
    y = np.sqrt(deg) * vec
    assert _sin(y, y_ref) <= 64 * 130 * EPS64 / (lam[2] - lam[1]) and float(y @ y_ref) > 0
    monkeypatch.setattr(ncut, "_fiedler", _NaNFirst(wrap.real, bad=2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(RuntimeError, match="non-finite"):
            ncut.second_smallest_eigenvector(Ab, db, eps)


def test_cut_loop_retries_a_non_finite_eigenvector(device, monkeypatch):
    from unscene3d_amd.pseudo_masks import ncut

    S = 130
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(S, 48, generator=g).to(device)
    segs = torch.arange(S)
    conn = torch.tensor([[i, i + 1] for i in range(S - 1)] + [[i + 1, i] for i in range(S - 1)], dtype=torch.int64)

    def one_iteration():
        seen = []
        gen = ncut.unscene3d_steps(feats, segs, conn, max_number_of_instances=1, min_segment_size=1,
                                   eigvec_hook=lambda it, v: seen.append(v.copy()) or v)
        next(gen).synchronize()
        with pytest.raises(StopIteration) as done:
            next(gen)
        return seen, done.value.value

    (clean,), masks = one_iteration()
    assert np.isfinite(clean).all()
    wrap = _NaNFirst(ncut._fiedler, bad=1)
    monkeypatch.setattr(ncut, "_fiedler", wrap)
    with pytest.warns(RuntimeWarning, match="stepwise"):
        (vec,), masks2 = one_iteration()
    assert wrap.calls == [False, True]
    assert np.array_equal(vec, clean) and np.array_equal(masks, masks2)
    monkeypatch.setattr(ncut, "_fiedler", _NaNFirst(wrap.real, bad=2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(RuntimeError, match="non-finite"):
            one_iteration()
