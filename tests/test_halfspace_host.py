"""CPU checks of the half-space and corridor limit factors (GVI_PSI_HINGE_HALFSPACE): the closed form of
tests/halfspace_ref.py against the box closed form of tests/box_ref.py by a rotation of the coordinates and on axis rows, and
against a dense product rule; the functions the kernels call (gaussianvi_amd/csrc/halfspace_moments.hpp) compiled for the host
under AddressSanitizer / UBSan against halfspace_ref, with the row convention of the root S; the builders; the shim call site."""
import os
import subprocess

import numpy as np
import pytest

import box_ref as br
import gvi_oracle as o
import halfspace_ref as hr
from gaussianvi_amd import api, build, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("E_phi", "cost", "Vdmu", "Vddmu", "E_xmuphi", "E_xxphi")
TS = [-6.0, -4.0, -2.5, -1.0, -0.3, 0.0, 0.3, 1.0, 2.5, 4.0, 6.0]


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


def test_constants():
    assert api.PSI_HINGE_HALFSPACE == 11 == syn.PSI_HINGE_HALFSPACE
    text = open(os.path.join(ROOT, "include", "gvi_hip.h")).read()
    assert "GVI_PSI_HINGE_HALFSPACE = 11" in text and "GVI_HALFSPACE_MAX_J = 16" in text


def rotation_onto_e1(a):
    """Orthogonal R with R a = |a| e_1 (a Householder reflection)."""
    d = len(a)
    u = a / np.linalg.norm(a)
    w = u - np.eye(d)[0]
    if np.linalg.norm(w) < 1e-14:
        return np.eye(d)
    w = w / np.linalg.norm(w)
    return np.eye(d) - 2.0 * np.outer(w, w)


def box_moments_of_row(a, b, sigma, eps, mu, Sigma, temperature):
    """The moments of sigma max(0, a^T x - (b - eps))^2 from box_ref: in y = R x the row is the upper limit hi = b / |a| (eps / |a|,
    sigma |a|^2) on coordinate 1 of a box without any other limit; moments rotate back as vectors and matrices."""
    d, na = len(a), np.linalg.norm(a)
    R = rotation_onto_e1(a)
    inf = np.full(d, np.inf)
    hi = inf.copy()
    hi[0] = b / na
    prm = syn.box_params(np.r_[sigma * na * na, np.ones(d - 1)], np.r_[eps / na, np.zeros(d - 1)], -inf, hi)
    r = br.closed_moments(prm, d, (R @ mu)[None], (R @ Sigma @ R.T)[None], temperature)
    return dict(E_phi=r["E_phi"][0], cost=r["cost"][0], Vdmu=R.T @ r["Vdmu"][0], Vddmu=R.T @ r["Vddmu"][0] @ R,
                E_xmuphi=R.T @ r["E_xmuphi"][0], E_xxphi=R.T @ r["E_xxphi"][0] @ R)


@pytest.mark.parametrize("d", [2, 3, 6])
def test_closed_form_vs_box_closed_form_by_rotation(d):
    """One row at every t of TS, then J = 3 rows by linearity: 1e-12 relative (max-norm per quantity)."""
    rng = np.random.default_rng(160 + d)
    worst = 0.0
    for t in TS:
        mu, Sigma = syn.random_marginals(rng, 1, d, 0.3)
        J = 3
        A = rng.normal(size=(J, d))
        sig, eps = rng.uniform(0.5, 4.0, J), rng.uniform(0.0, 0.2, J)
        sd = np.sqrt(np.einsum("ja,ab,jb->j", A, Sigma[0], A))
        tj = np.array([t, -0.5 * t, 0.4])
        b = A @ mu[0] + eps - tj * sd                       # gap = t sd
        assert np.allclose(hr.t_values(syn.halfspace_params(sig, eps, b, A), d, mu, Sigma)[0], tj, rtol=1e-9, atol=1e-12)
        for rows in ([0], [0, 1, 2]):
            prm = syn.halfspace_params(sig[rows], eps[rows], b[rows], A[rows])
            got = hr.closed_moments(prm, d, mu, Sigma, 1.7)
            parts = [box_moments_of_row(A[j], b[j], sig[j], eps[j], mu[0], Sigma[0], 1.7) for j in rows]
            for k in KEYS:
                ref = sum(part[k] for part in parts)
                err = relmax(got[k][0], ref)
                worst = max(worst, err)
                assert err <= 1e-12, (d, t, rows, k, err)
    print(f"d {d}: worst against the rotated box closed form {worst:.2e}")


def test_closed_form_vs_dense_product_rule():
    """d = 2 with a correlated Sigma and oblique rows: the closed moments against a 200 x 200 product Gauss-Hermite rule.  The rule
    converges algebraically on a kink; 2e-4 is the bound of the box test of the same name."""
    x, w = np.polynomial.hermite_e.hermegauss(200)
    w = w / w.sum()
    Z = np.stack(np.meshgrid(x, x, indexing="ij"), axis=-1).reshape(-1, 2)
    W = np.outer(w, w).reshape(-1)
    rng = np.random.default_rng(12)
    mu, Sigma = syn.random_marginals(rng, 3, 2, 0.1)
    A = np.array([[1.0, 1.0], [-1.0, 0.5], [0.2, -1.0]])
    prm = syn.halfspace_params(rng.uniform(1, 5, (3, 3)), 0.1, [1.0, 1.0, 1.0], A)
    mu[:] = [[0.5, 0.45], [-0.9, 0.3], [0.1, -1.3]]
    ref = o.batched_moments(Z, W, mu, Sigma, hr.psi_batch(prm, 2), 1.5)
    got = hr.closed_moments(prm, 2, mu, Sigma, 1.5)
    assert np.nanmin(np.abs(hr.t_values(prm, 2, mu, Sigma))) < 1.0          # a kink inside the bulk of the Gaussian
    for k in ("E_phi", "Vdmu", "Vddmu", "E_xmuphi", "E_xxphi"):
        err = np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()
        print(k, f"{err:.2e}")
        assert err <= 2e-4, (k, err)


@pytest.mark.parametrize("d", [1, 2, 4, 8])
def test_axis_rows_give_the_box_numbers(d):
    """Rows +e_i (b = hi_i) and -e_i (b = -lo_i) are the box of the same limits: box_ref's numbers to rounding."""
    rng = np.random.default_rng(170 + d)
    K = 4
    mu, Sigma = syn.random_marginals(rng, K, d, 0.2)
    sig, eps = rng.uniform(1.0, 5.0, (K, d)), rng.uniform(0.0, 0.2, (K, d))
    lo, hi = -rng.uniform(0.2, 1.0, (K, d)), rng.uniform(0.2, 1.0, (K, d))
    box = syn.box_params(sig, eps, lo, hi)
    A = np.concatenate([np.eye(d), -np.eye(d)])
    half = syn.halfspace_params(np.concatenate([sig, sig], axis=1), np.concatenate([eps, eps], axis=1), np.concatenate([hi, -lo], axis=1), A)
    assert half.shape == (K, 2 * d * (d + 3))
    T = rng.uniform(0.5, 3.0, K)
    got, ref = hr.closed_moments(half, d, mu, Sigma, T), br.closed_moments(box, d, mu, Sigma, T)
    for k in KEYS:
        assert relmax(got[k], ref[k]) <= 1e-13, (k, relmax(got[k], ref[k]))
    X = mu[:, None, :] + rng.normal(size=(K, 7, d))
    assert relmax(hr.psi_batch(half, d)(X), br.psi_batch(box, d)(X)) <= 1e-15
    assert np.array_equal(hr.margin(half, d, X), br.margin(box, d, X))


# ---- the header on the CPU ----
def sym_root(Sigma):
    lam, V = np.linalg.eigh(Sigma)
    return (V * np.sqrt(np.maximum(lam, 0.0))) @ V.T


def stub_cases():
    """(d, J, params [J (d + 3)], mu, Sigma, roots, x, tag): a grid of (d, J, t) with about a quarter of the rows off, then the edges.
    t stays off -3 (and -3 / 0.6): box_side and box_ref switch formulas there, and the rounding of t = gap / sd -- sd comes from a
    root on one side and from a^T Sigma a on the other -- would decide which branch each takes."""
    rng = np.random.default_rng(16)
    cases = []
    for d in (1, 2, 3, 6, 8):
        for J in (1, 3, 16):
            for t in (-9.0, -6.0, -3.5, -2.5, -1.0, 0.0, 1e-9, 0.7, 2.5, 6.0):
                mu, Sigma = syn.random_marginals(rng, 1, d, 0.3)
                A = rng.normal(size=(J, d))
                sig, eps = rng.uniform(0.5, 4.0, J), rng.uniform(0.0, 0.2, J)
                if J > 1:
                    off = rng.random(J) < 0.25
                    sig[off] = 0.0
                    A[off & (rng.random(J) < 0.5)] = 0.0             # an off row may carry a zero normal
                sd = np.sqrt(np.einsum("ja,ab,jb->j", A, Sigma[0], A))
                tj = t * np.where(np.arange(J) % 2 == 0, 1.0, -0.6)
                b = A @ mu[0] + eps - tj * sd
                x = mu[0] + rng.normal(size=d) * 0.5
                cases.append((d, J, syn.halfspace_params(sig, eps, b, A)[0], mu[0], Sigma[0], None, x, "grid"))
    # t = +-40 on single rows; an all-off factor; sd = 0: a row orthogonal to the range of a singular Sigma
    for t in (40.0, -40.0):
        mu, Sigma = syn.random_marginals(rng, 1, 3, 0.3)
        a = rng.normal(size=(1, 3))
        sd = np.sqrt(a[0] @ Sigma[0] @ a[0])
        cases.append((3, 1, syn.halfspace_params(2.0, 0.1, a @ mu[0] + 0.1 - t * sd, a)[0], mu[0], Sigma[0], None, mu[0] + 0.1, f"t{t:+.0f}"))
    mu, Sigma = syn.random_marginals(rng, 1, 4, 0.3)
    cases.append((4, 3, syn.halfspace_params(0.0, 0.1, 1.0, np.r_[rng.normal(size=(2, 4)), np.zeros((1, 4))])[0], mu[0], Sigma[0], None, mu[0], "alloff"))
    Sing = np.diag([0.09, 0.0, 0.04])
    L = np.diag([0.3, 0.0, 0.2])
    for gap in (0.25, -0.25):
        A = np.array([[0.0, 2.0, 0.0], [1.0, 1.0, 0.0]])
        m = np.array([0.1, 0.5, -0.2])
        b = np.array([A[0] @ m + 0.1 - gap, 0.9])
        cases.append((3, 2, syn.halfspace_params([3.0, 1.5], 0.1, b, A)[0], m, Sing, (L, L), m, f"sd0{gap:+.2f}"))
    return cases


def test_device_functions_on_cpu_under_sanitizers(tmp_path):
    """halfspace_moments.hpp as a stand-alone host program built with -fsanitize=address,undefined, run on stub_cases() TWICE: with
    the symmetric root of Sigma and with its lower Cholesky factor, both row-major with x = mu + S z.
      rows: (e0, e1, e2) against halfspace_ref at 1e-13 relative to the value, entry by entry (below 1e-300 on both sides at
            t = -40), the bound of the box program's test;
      moments: S m1 and S (M2 - m0 I) S^T + m0 Sigma of the two roots agree with each other and with halfspace_ref to 1e-12
            (max-norm relative).  With rows and columns of S swapped (v = S a instead of S^T a) the Cholesky run is wrong in the
            first digit: that is what this part is for;
      psi and margin at a point: 1e-15 / 1e-13."""
    exe = str(tmp_path / "halfspace_on_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "gaussianvi_amd", "csrc"), os.path.join(ROOT, "tests", "stubs", "halfspace_on_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = stub_cases()
    assert {c[1] for c in cases} >= {1, 3, 16}
    runs = {}
    for which in (0, 1):
        path = str(tmp_path / f"cases{which}.txt")
        with open(path, "w") as f:
            f.write(f"{len(cases)}\n")
            for d, J, prm, mu, Sigma, roots, x, _ in cases:
                S = roots[which] if roots is not None else (sym_root(Sigma) if which == 0 else np.linalg.cholesky(Sigma))
                if which == 1 and d > 1 and roots is None:
                    assert np.abs(S - S.T).max() > 1e-3                  # a root whose rows and columns differ
                f.write(f"{d} {J}\n" + "\n".join(" ".join(float(v).hex() for v in np.ravel(arr)) for arr in (prm, mu, S, x)) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ALL OK"), r.stdout[-2000:] + r.stderr[-4000:]
        runs[which] = [ln.split() for ln in r.stdout.splitlines()]
    worst_row, worst_mom, worst_roots = 0.0, 0.0, 0.0
    moms = {}
    for which, lines in runs.items():
        rows = {(int(t[1]), int(t[2])): np.array([float.fromhex(v) for v in t[3:]]) for t in lines if t[0] == "row"}
        mom = {int(t[1]): np.array([float.fromhex(v) for v in t[2:]]) for t in lines if t[0] == "mom"}
        point = {int(t[1]): [float.fromhex(v) for v in t[2:]] for t in lines if t[0] == "point"}
        assert len(mom) == len(point) == len(cases) and len(rows) == sum(c[1] for c in cases)
        for ci, (d, J, prm, mu, Sigma, roots, x, tag) in enumerate(cases):
            S = roots[which] if roots is not None else (sym_root(Sigma) if which == 0 else np.linalg.cholesky(Sigma))
            P = prm[None]
            e = [v[0] for v in hr.row_expectations(P, d, mu[None], Sigma[None])]
            for j in range(J):
                got, ref = rows[(ci, j)], np.array([e[0][j], e[1][j], e[2][j]])
                assert np.isfinite(got).all()
                if prm[j] == 0.0:
                    assert (got == 0).all()
                    continue
                if tag.startswith("sd0") and j == 0:                    # deterministic scalar: the hinge at the mean, exactly
                    g = max(float(tag[3:]), 0.0)
                    assert np.allclose(got, [3.0 * g * g, 6.0 * g, 6.0 if g > 0 else 0.0], rtol=1e-15, atol=0), (tag, got)
                tiny = np.abs(ref) < 1e-300
                assert (np.abs(got[tiny]) < 1e-300).all(), (tag, ci, j, got, ref)
                err = np.abs(got[~tiny] - ref[~tiny]) / np.abs(ref[~tiny])
                if err.size:
                    worst_row = max(worst_row, err.max())
                    assert err.max() <= 1e-13, (tag, which, d, J, j, got, ref)
            if tag == "t-40":
                assert np.abs(mom[ci]).max() <= 1e-300
            if tag == "alloff":
                assert (mom[ci] == 0).all() and point[ci] == [0.0, np.inf]
            m0, m1, M2 = mom[ci][0], mom[ci][1:1 + d], mom[ci][1 + d:].reshape(d, d)
            back = dict(E_phi=m0, E_xmuphi=S @ m1, E_xxphi=S @ M2 @ S.T)
            ref = hr.closed_moments(P, d, mu[None], Sigma[None], 1.0)
            for k, v in back.items():
                err = relmax(v, ref[k][0])
                worst_mom = max(worst_mom, err)
                assert err <= 1e-12, (tag, which, d, J, k, err)
            moms[(which, ci)] = back
            X = x[None, None, :]
            psi_ref, mg_ref = hr.psi_batch(P, d)(X)[0, 0], hr.margin(P, d, X)[0, 0]
            # rounding of e_j = a_j^T x - (b_j - eps_j), on each side: de <= (d + 2) u (sum_i |a_ji x_i| + |b_j| + |eps_j|), u = 2^-53;
            # psi = sum sigma e^2 moves by sum sigma 2 |e| de, the margin by de / |a_j| of some row
            sg, ep, bb, AA = (v[0] for v in hr.unpack(P, d))
            de = 2 * (d + 2) * 2.0 ** -53 * (np.abs(AA) @ np.abs(x) + np.abs(bb) + np.abs(ep))
            ee = np.maximum(AA @ x - (bb - ep), 0.0) + de
            assert abs(point[ci][0] - psi_ref) <= (sg * 2 * ee * de).sum() + 4 * J * 2.0 ** -53 * psi_ref
            on = sg > 0
            assert point[ci][1] == mg_ref or abs(point[ci][1] - mg_ref) <= (de[on] / np.linalg.norm(AA[on], axis=1)).max() + 4 * 2.0 ** -53 * abs(mg_ref)
    for ci in range(len(cases)):
        for k in ("E_phi", "E_xmuphi", "E_xxphi"):
            err = relmax(moms[(1, ci)][k], moms[(0, ci)][k])
            worst_roots = max(worst_roots, err)
            assert err <= 1e-12, (cases[ci][7], k, err)
    print(f"host build of halfspace_moments.hpp: rows {worst_row:.2e}, moments {worst_mom:.2e}, Cholesky against symmetric root {worst_roots:.2e}")


def test_row_convention_is_visible():
    """The check above can see a transposed root: the numpy moments formed with v = S a instead of S^T a differ from the reference by
    far more than its bound for a Cholesky factor, and not at all for the symmetric root."""
    rng = np.random.default_rng(5)
    mu, Sigma = syn.random_marginals(rng, 1, 4, 0.3)
    a = rng.normal(size=4)
    ref_sd = np.sqrt(a @ Sigma[0] @ a)
    L, R = np.linalg.cholesky(Sigma[0]), sym_root(Sigma[0])
    assert abs(np.linalg.norm(L.T @ a) - ref_sd) <= 1e-14 * ref_sd and abs(np.linalg.norm(R @ a) - ref_sd) <= 1e-14 * ref_sd
    assert abs(np.linalg.norm(L @ a) - ref_sd) > 1e-3 * ref_sd


def test_halfspace_params_and_builders():
    prm = syn.halfspace_params([2.0, 3.0], 0.1, [1.0, -1.0], [[1.0, 0.0, 0.5], [0.0, -1.0, 0.0]])
    assert prm.shape == (1, 12) and prm.flags["C_CONTIGUOUS"]
    assert np.array_equal(prm[0], [2.0, 3.0, 0.1, 0.1, 1.0, -1.0, 1.0, 0.0, 0.5, 0.0, -1.0, 0.0])
    pad = syn.halfspace_params([2.0, 3.0], 0.1, [1.0, -1.0], [[1.0, 0.0, 0.5], [0.0, -1.0, 0.0]], J=4)
    assert pad.shape == (1, 24)
    sig, eps, b, A = hr.unpack(pad, 3)
    assert np.array_equal(sig[0], [2.0, 3.0, 0.0, 0.0]) and np.array_equal(eps[0], [0.1, 0.1, 0.0, 0.0]) and (A[0, 2:] == 0).all()
    assert np.array_equal(A[0, :2], [[1.0, 0.0, 0.5], [0.0, -1.0, 0.0]]) and np.array_equal(b[0], [1.0, -1.0, 0.0, 0.0])
    # per factor: [K][J][d] with [K][J] scalars, and a ragged list padded to the largest row count
    per = syn.halfspace_params(np.array([[1.0, 2.0], [3.0, 4.0]]), 0.0, 1.0, np.arange(12.0).reshape(2, 2, 3))
    assert per.shape == (2, 12) and np.array_equal(per[1], [3.0, 4.0, 0.0, 0.0, 1.0, 1.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0])
    rag = syn.halfspace_params([[1.0], [2.0, 3.0, 4.0]], 0.05, [[0.5], [1.0, 2.0, 3.0]], [np.ones((1, 2)), np.arange(6.0).reshape(3, 2)])
    assert rag.shape == (2, 15)
    sig, eps, b, A = hr.unpack(rag, 2)
    assert np.array_equal(sig, [[1.0, 0.0, 0.0], [2.0, 3.0, 4.0]]) and np.array_equal(b[0], [0.5, 0.0, 0.0]) and (A[0, 1:] == 0).all()
    assert np.array_equal(eps, [[0.05, 0.0, 0.0], [0.05, 0.05, 0.05]]) and np.array_equal(A[1], np.arange(6.0).reshape(3, 2))
    # an off row adds nothing and is skipped in the margin
    X = np.random.default_rng(0).normal(size=(2, 5, 2))
    assert np.array_equal(hr.psi_batch(rag, 2)(X)[0], hr.psi_batch(rag[:1, [0, 3, 6, 9, 10]], 2)(X[:1])[0])
    assert np.array_equal(hr.margin(rag, 2, X)[0], (0.5 - X[0].sum(axis=1)) / np.sqrt(2.0))

    base = syn.make_planar_chain(T=9)
    normals = np.array([[0.0, 1.0], [0.0, -1.0], [1.0, 0.0], [-1.0, 0.0]])
    ch = syn.add_corridor_set(base, normals, [0.5, 0.5, 4.0, 4.0], sigma=8.0, eps=0.05, p=4)
    assert len(ch["specs"]) == len(base["specs"]) + 1 and all(a is b for a, b in zip(ch["specs"], base["specs"]))
    assert len(base["specs"]) == 3                                       # the chain it was built from is left alone
    cor = ch["specs"][-1]
    assert (cor["kind"], cor["d"], cor["p"], cor["params"].shape) == (syn.PSI_HINGE_HALFSPACE, 4, 4, (9, 28))
    assert np.array_equal(cor["start"], np.arange(9)) and (cor["temperature"] == 1).all()
    sig, eps, b, A = hr.unpack(cor["params"], 4)
    assert (sig == 8).all() and (eps == 0.05).all() and np.array_equal(A[3, :, :2], normals) and (A[:, :, 2:] == 0).all()
    # one polygon per state
    offs = np.tile([0.5, 0.5, 4.0, 4.0], (9, 1)) + np.arange(9)[:, None] * 0.1
    per = syn.add_corridor_set(base, np.stack([normals] * 9), offs)["specs"][-1]
    assert np.array_equal(hr.unpack(per["params"], 4)[2], offs)
    # pair = True: the rows reproduce n^T (W x + c) <= b at every tau
    dt, taus = 0.25, [0.05, 0.125, 0.2]
    pair = syn.add_corridor_set(base, normals, [0.5, 0.5, 4.0, 4.0], pair=True, taus=taus, dt=dt)["specs"][-1]
    assert (pair["d"], pair["params"].shape) == (8, (8, 12 * 11)) and np.array_equal(pair["start"], np.arange(8))
    W, c = syn.minacc_segment_readout(2, syn.QC, dt, taus, 2)
    sig, eps, b, A = hr.unpack(pair["params"], 8)
    x = np.random.default_rng(1).normal(size=8)
    for l in range(3):
        pos = W[l] @ x + c[l]
        for j in range(4):
            assert np.isclose(A[5, 4 * l + j] @ x - b[5, 4 * l + j], normals[j] @ pos - [0.5, 0.5, 4.0, 4.0][j], rtol=0, atol=1e-13)
    mid = syn.add_corridor_set(base, normals, [0.5, 0.5, 4.0, 4.0], pair=True)["specs"][-1]
    assert mid["params"].shape == (8, 4 * 11)
    Ai, Bi, _ = syn.minacc_interpolation(2, syn.QC, 0.25, 0.125)
    assert np.allclose(hr.unpack(mid["params"], 8)[3][0, 0], np.r_[Ai[1], Bi[1]], rtol=0, atol=1e-15)       # row n = (0, 1): the y read-out


def test_oracle_accepts_the_closed_form():
    """o.ChainNGD on planar(T = 9) plus the corridor, closed form plugged in as fast_moments: the first step is accepted."""
    import test_halfspace_gpu as g
    ch = g.corridor_graph(False)
    ngd = o.ChainNGD(ch["T"], ch["n"], ch["oracle_sets"](True), ch["mu0"], ch["D0"], ch["U0"])
    ok, cost, ntr = ngd.step()
    print(f"accepted {ok} cost {cost:.4f} trials {ntr}")
    assert ok


def test_callsite_compiles_against_the_shim(tmp_path):
    build.build_lib()
    exe = str(tmp_path / "halfspace_callsite")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "stubs", "halfspace_callsite.cpp"), "-L", os.path.join(ROOT, "gaussianvi_amd"), "-lgvi_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "gaussianvi_amd"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
