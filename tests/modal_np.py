"""NumPy statement of the modal solve: the lowest positive pairs of  A phi = mu M phi,  A = K + sigma M, on
the free DOFs by LOBPCG, step for step what tlfea_newton_modal_solve runs on the device -- the same start block, the same
masking, the same Rayleigh-Ritz on S = [X W P], the same soft locking and the same convergence test.  Only the
preconditioner differs: T here is the inverse of the 3 x 3 node blocks of A (block-Jacobi), the engine applies the Newton
solver's polynomial / p-multigrid cycle.

A is SPD; M need not be: the consistent T10 mass matrix of the 5-point Keast rule (one negative weight) has negative and
zero eigenvalues.  So the block is kept A-orthonormal and the Rayleigh-Ritz step takes the LARGEST theta = 1 / mu of
M c = theta A c -- the physical modes are the pairs with the largest theta, whatever the sign structure of M.  The modes
are returned M-normalised (phi^T M phi = 1, theta > 0).

    start   X = hash(dof, column, seed) in [-1, 1), zero on pinned rows, Rayleigh-Ritz on X alone (X^T A X = I)
    repeat  R = A X - M X diag(mu)                 column i converged:  mu_i > 0 and ||r_i|| <= tol mu_i ||M x_i||
            W = T R (unconverged columns only), masked,  W -= X (AX^T W)
            A W, M W                               the one block product with each matrix per iteration
            G_A = S^T A S,  G_M = S^T M S          S = [X W P], the columns in use
            G_M c = theta G_A c                    unit-diagonal scaling, Cholesky of G_A, SVQB where that breaks down
            X, P (and A X, A P, M X, M P) <- S C   P = the W and P part of the new X
    finish  A X, M X recomputed from X before convergence is declared (the recurrences drift)
"""
import numpy as np

CHOL_PIVOT_MIN = 1e-10   # smallest pivot of the unit-diagonal Gram matrix the Cholesky path accepts
SVQB_DROP = 1e-12        # SVQB: directions of the unit-diagonal Gram matrix below this share of its largest eigenvalue go


def hash_block(n, m, seed):
    """[n, m] start block: splitmix64 of (dof, column, seed), top 53 bits mapped to [-1, 1)."""
    dof = np.arange(n, dtype=np.uint64)[:, None]
    col = np.arange(m, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        z = dof * np.uint64(0x9E3779B97F4A7C15) + col * np.uint64(0xD1B54A32D192ED03) + \
            np.uint64(seed) * np.uint64(0x94D049BB133111EB) + np.uint64(0x2545F4914F6CDD1D)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0


def cholesky_lower(G, pivot_min):
    """Lower Cholesky factor of G, or None when a pivot falls to pivot_min or below."""
    k = G.shape[0]
    L = np.zeros_like(G)
    for j in range(k):
        d = G[j, j] - L[j, :j] @ L[j, :j]
        if not d > pivot_min:
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (G[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def jacobi_eigh(A):
    """Eigenvalues (ascending) and vectors of a symmetric matrix (the engine runs cyclic Jacobi rotations here)."""
    return np.linalg.eigh(A)


def rayleigh_ritz(GA, GM, n_want):
    """The n_want pairs of GM c = theta GA c with the largest theta (both symmetric, GA positive definite up to rank
    loss of the basis): -> theta (descending), C with C^T GA C = I.  GA is scaled to unit diagonal; its Cholesky factor
    where every pivot stays above CHOL_PIVOT_MIN, else SVQB (eigen-decomposition of the scaled GA, small directions
    dropped)."""
    GA, GM = 0.5 * (GA + GA.T), 0.5 * (GM + GM.T)
    d = 1.0 / np.sqrt(np.diag(GA))
    B = GA * d[:, None] * d[None, :]
    L = cholesky_lower(B, CHOL_PIVOT_MIN)
    if L is not None:
        Q = np.linalg.inv(L).T * d[:, None]            # Q^T GA Q = I
    else:
        w, V = jacobi_eigh(B)
        keep = w > SVQB_DROP * w[-1]
        Q = (V[:, keep] / np.sqrt(w[keep])[None, :]) * d[:, None]
    th, Z = jacobi_eigh(Q.T @ GM @ Q)
    n_want = min(n_want, len(th))
    return th[::-1][:n_want].copy(), Q @ Z[:, ::-1][:, :n_want]


def mu_of(theta):
    """mu = 1 / theta (0 where theta is 0: such a column is never a converged one)"""
    return np.where(theta != 0.0, 1.0 / np.where(theta != 0.0, theta, 1.0), 0.0)


def block_jacobi(A, n_nodes):
    """T r: the inverse 3 x 3 node blocks of the (scipy sparse or dense) matrix A."""
    A = np.asarray(A.todense()) if hasattr(A, "todense") else np.asarray(A)
    inv = np.stack([np.linalg.inv(A[3 * i:3 * i + 3, 3 * i:3 * i + 3]) for i in range(n_nodes)])

    def apply(r):
        return np.einsum("nij,nj->ni", inv, r.reshape(n_nodes, 3)).reshape(-1)
    return apply


def lobpcg(A, M, T, free, n_modes, block_extra=None, tol=1e-8, max_iter=500, seed=0):
    """A, M: matrices (anything with @) on all n DOFs; T: callable r -> T r; free: bool [n], False on pinned rows.
    -> dict(mu, modes [n, n_modes], resid, iterations, converged, block)."""
    n = len(free)
    if block_extra is None:
        block_extra = default_block_extra(n_modes)
    m = n_modes + block_extra
    assert 1 <= n_modes and m <= 32 and 3 * m <= int(free.sum())
    mask = free.astype(np.float64)[:, None]
    S = np.zeros((n, 3 * m))
    S[:, :m] = hash_block(n, m, seed) * mask
    AS, MS = np.zeros_like(S), np.zeros_like(S)
    MS[:, :m] = (M @ S[:, :m]) * mask
    AS[:, :m] = (A @ S[:, :m]) * mask
    idx = np.arange(m)
    theta, C = rayleigh_ritz(S[:, idx].T @ AS[:, idx], S[:, idx].T @ MS[:, idx], m)
    mu = mu_of(theta)
    for Z in (S, AS, MS):
        Z[:, :m] = Z[:, idx] @ C
    p_valid = np.zeros(m, dtype=bool)                    # columns of P that hold a direction
    it = 0
    verified = False
    while True:
        R = AS[:, :m] - MS[:, :m] * mu[None, :]
        rn, mn = np.sqrt(np.sum(R * R, axis=0)), np.sqrt(np.sum(MS[:, :m] ** 2, axis=0))
        conv = (theta > 0.0) & (rn <= tol * mu * mn)
        if conv[:n_modes].all():
            if verified:
                break
            # the products kept by recurrence drift: declare convergence on recomputed ones only
            MS[:, :m] = (M @ S[:, :m]) * mask
            AS[:, :m] = (A @ S[:, :m]) * mask
            verified = True
            continue
        verified = False
        if it == max_iter:
            break
        it += 1
        act = np.where(~conv)[0]
        S[:, m:2 * m] = 0.0
        for j in act:
            S[:, m + j] = T(R[:, j]) * mask[:, 0]
        S[:, m:2 * m] -= S[:, :m] @ (AS[:, :m].T @ S[:, m:2 * m])
        AS[:, m:2 * m] = (A @ S[:, m:2 * m]) * mask
        MS[:, m:2 * m] = (M @ S[:, m:2 * m]) * mask
        GA, GM = S.T @ AS, S.T @ MS
        idx = np.concatenate([np.arange(m), m + act, 2 * m + np.where(~conv & p_valid)[0]])
        theta, Ck = rayleigh_ritz(GA[np.ix_(idx, idx)], GM[np.ix_(idx, idx)], m)
        mu = mu_of(theta)
        C = np.zeros((3 * m, m))
        C[idx] = Ck
        Cp = C.copy()
        Cp[:m] = 0.0
        Cp[:, conv] = 0.0                                # a locked column keeps no search direction
        for Z in (S, AS, MS):
            Xn, Pn = Z @ C, Z @ Cp
            Z[:, :m], Z[:, 2 * m:] = Xn, Pn
        p_valid = ~conv
    ok = theta[:n_modes] > 0.0
    scale = np.where(ok, 1.0 / np.sqrt(np.where(ok, theta[:n_modes], 1.0)), 0.0)   # x^T A x = 1, x^T M x = theta
    rel = np.where(ok, rn[:n_modes] / np.where(ok, mu[:n_modes] * mn[:n_modes], 1.0), np.inf)
    return dict(mu=mu[:n_modes].copy(), modes=S[:, :n_modes] * scale[None, :], resid=rel, iterations=it,
                converged=int(conv[:n_modes].sum()), block=m)


def default_block_extra(n_modes):
    """guard columns of the block when the caller names none: half the wanted modes, at least 2, within the cap of 32"""
    return max(0, min(max(2, n_modes // 2), 32 - n_modes))
