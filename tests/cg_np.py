"""Step-by-step check of a CG trace (SyncedNewtonSolver.CGTrace, or a numpy PCG that writes the same records) against
fp64 / long-double restatements of each kernel of the iteration.

Every check is LOCAL: iteration i is judged from the trace's own iterates before it, so round-off is never carried from
step to step and a bound is the round-off of ONE kernel.  u = 2^-53, |.| entrywise, references in np.longdouble.

Records (as tlfea_newton_cg_trace writes them): record 0 after the start (x = 0, r = b), record i + 1 after iteration i.
  x_i, r_i   = rec[i].x, rec[i].r
  p_i, q_i   = rec[i + 1].p, rec[i + 1].q
  z_i        = rec[i].z with the block-Jacobi update (form.update 0: the update kernel already wrote z of the new r),
               rec[i + 1].z with a polynomial preconditioner (z is formed at the start of iteration i)
  rz_i       = rec[i + 1].sums[i & 1], pq_i = rec[i + 1].sums[2], rr_{i+1} = rec[i + 1].sums[3]

Bounds (none is tuned to a device):
  product    |q_i - H p_i|_row <= (nnz_row + 4) u (|H||p_i|)_row: a sum of nnz_row = 3 deg products in any order, plus slack
             for a p formed on the fly.  Mixed-precision iteration: H is H.astype(float32) widened back.  Matrix-free
             product: max |q - H p| <= 1e-12 max |H p| (the bound of tests/test_gpu_matfree.py).
  direction  p_0 = z_0 bit for bit; |p_i - (z_i + beta p_{i-1})| <= 32 u (|z_i| + |beta p_{i-1}|), beta = rz_i / rz_{i-1}
             from the returned sums (32 u: the kernels add the 512 slots in another order than the sums returned).
  update     the same form for x_{i+1} = x_i + alpha p_i and r_{i+1} = r_i - alpha q_i, alpha = rz_i / pq_i.  After a residual
             replacement r_{i+1} meets the product bound against b - H x_{i+1} instead.  The replacement's own product
             reuses the q buffer, so the record of that iteration holds q = H x_{i+1} (fp64 H) and not q_i: it is held to the
             product bound against H x_{i+1}, r_{i+1} = b - q to one rounding, and the p.q sum -- all that is left of q_i --
             to the dot bound plus p_i . (the product bound of the working operator) against the long-double p_i . (H p_i).
  dots       |sum - long-double dot| <= (L + 2) u sum |a_j b_j|, L the longest addition chain: per-thread loop (from the
             launchers' grids below) + wave butterfly 6 + LDS hop 16 + slot loop 2 + butterfly 6 + LDS hop 16.  Slots at or
             beyond the grid of the kernel that wrote them are exactly 0.
  z          block-Jacobi: |z - D^-1 r|_c <= 8 u (|D^-1||r|)_c with D^-1 restated from H.  Polynomial / p-multigrid: the
             caller passes the restated operator and the bound of tests/test_gpu_precond_operator.py.
"""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
LD = np.longdouble
NPART = 512
TAIL = 6 + 16 + 2 + 6 + 16   # butterfly, LDS hop, slot loop, second butterfly, second LDS hop


class TraceError(AssertionError):
    pass


def ceil_div(a, b):
    return -(-int(a) // int(b))


# ---- the launchers' geometry (csrc/solver_kernels.hip, csrc/elem_kernels.hip), restated -------------------------------
def spmv_grid(N):
    return max(1, min(NPART, ceil_div(N, 32)))


def slot_grid_256(n):
    return max(1, min(NPART, ceil_div(n, 256)))


def matfree_grid(N):
    return max(1, min(NPART, ceil_div(N, 128)))


def loop_terms(N, form):
    """per-thread addition chains of the four reductions, from the launchers' grids: dict(pq, rr, rz, init)"""
    G = 1024 // form["lanes"]
    if form["matfree"]:
        g = matfree_grid(N)
        pq = ceil_div(ceil_div(ceil_div(N, g), 128) * 128, 128)
    elif form["xcd"]:
        pq = ceil_div(ceil_div(ceil_div(N, 8), G) * G, (form["grid"] // 8) * G)
    elif form["tiled"]:
        pq = ceil_div(N, form["grid"] * G)
    else:
        pq = ceil_div(ceil_div(N, form["grid"]), G)
    ug = form["update_grid"]
    rr = ceil_div(3 * N, ug * 256) if form["update"] == 1 else 3 * ceil_div(N, ug * 256)
    if form["update"] == 0:
        rz = rr
    else:  # last step of the polynomial: one row per lane group and trip, at most 32 lanes per row, the eighths add a trip
        rz = ceil_div(N, max(1, min(NPART, ceil_div(N, 32))) * 32) + 1
    return dict(pq=pq, rr=rr, rz=rz, init=3 * ceil_div(N, NPART * 256))


# ---- long-double pieces -----------------------------------------------------------------------------------------------
def row_dot(H, v, absolute=False):
    """(H v)_row in long double (|H||v| in float64 when absolute), H scipy CSR with no empty row"""
    if absolute:
        return np.add.reduceat(np.abs(H.data) * np.abs(v)[H.indices], H.indptr[:-1])
    return np.add.reduceat(H.data.astype(LD) * v.astype(LD)[H.indices], H.indptr[:-1])


def dinv_blocks(H):
    """inverse 3 x 3 diagonal blocks of H in long double, [N, 3, 3]"""
    N = H.shape[0] // 3
    D = np.zeros((N, 3, 3), dtype=LD)
    coo = H.tocoo()
    m = (coo.row // 3) == (coo.col // 3)
    np.add.at(D, (coo.row[m] // 3, coo.row[m] % 3, coo.col[m] % 3), coo.data[m].astype(LD))
    c = np.empty_like(D)
    for a in range(3):
        for b in range(3):
            a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
            c[:, b, a] = D[:, a1, b1] * D[:, a2, b2] - D[:, a1, b2] * D[:, a2, b1]   # adjugate
    det = D[:, 0, 0] * c[:, 0, 0] + D[:, 0, 1] * c[:, 1, 0] + D[:, 0, 2] * c[:, 2, 0]
    return c / det[:, None, None]


def row_classes(H, lanes):
    """node rows with 3 deg < lanes (no second round), lanes < 3 deg < 2 lanes (a partial second round), 3 deg > 2 lanes
    (several passes): the three counts"""
    row = np.diff(H.indptr)[::3]
    return int((row < lanes).sum()), int(((row > lanes) & (row < 2 * lanes)).sum()), int((row > 2 * lanes).sum())


def _worst(err, bound, what, it, ratios, key):
    """ratio of the largest error to its bound; raises with the place of the worst entry"""
    err = np.asarray(err, dtype=np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    bad = err > bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, err / bound, np.where(err > 0.0, np.inf, 0.0))
    j = int(np.argmax(ratio)) if ratio.ndim else 0
    worst = float(ratio.max()) if ratio.ndim else float(ratio)
    ratios[key] = max(ratios.get(key, 0.0), worst)
    if np.any(bad):
        e, b = (err[j], bound[j]) if ratio.ndim else (err, bound)
        raise TraceError("%s, iteration %s: entry %d (node row %d) is off by %.3e, bound %.3e (%d entries beyond)"
                         % (what, it, j, j // 3, e, b, int(bad.sum())))


def _dot(ratios, key, what, it, got, a, b, L):
    prod = a.astype(LD) * b.astype(LD)
    ref, mag = prod.sum(), float(np.abs(prod).sum())
    _worst(abs(float(LD(got) - ref)), (L + 2) * U * mag, what, it, ratios, key)


def check_trace(H, b, tr, precond=None, z_bound=None, z_records=None):
    """Checks every iteration of the trace `tr` (dict of x, r, z, p, q [k+1, n], sums [k+1, 4], slots [k+1, 5, 512], form)
    of H x = b.  precond / z_bound: restated M^-1 and the relative 2-norm bound of z against it (polynomial forms; z_records:
    how many of the z to compare).  Returns the worst ratio of each measured error to its bound; raises TraceError naming
    kernel, iteration and row where a bound is missed."""
    H = sp.csr_matrix(H)
    n = H.shape[0]
    N = n // 3
    f = tr["form"]
    k = tr["x"].shape[0] - 1
    jac = f["update"] == 0
    nnz_row = np.diff(H.indptr).astype(np.float64)
    Hcg = sp.csr_matrix((H.data.astype(np.float32).astype(np.float64), H.indices, H.indptr), shape=H.shape) if f["spmv32"] else H
    loops = loop_terms(N, f)
    ratios = {}
    x, r, p, q, sums, slots = tr["x"], tr["r"], tr["p"], tr["q"], tr["sums"], tr["slots"]
    z_of = (lambda i: tr["z"][i]) if jac else (lambda i: tr["z"][i + 1])
    rz_of = lambda i: float(sums[i + 1, i & 1])
    Dinv = dinv_blocks(H) if jac else None

    # ---- the start ------------------------------------------------------------------------------------------------
    if np.any(x[0] != 0.0) or not np.array_equal(r[0], b):
        raise TraceError("start: x_0 = 0, r_0 = b does not hold")
    _dot(ratios, "dot", "start r.z sum", 0, sums[0, 0], r[0], tr["z"][0], loops["init"] + TAIL)

    def check_z_jacobi(i, zi, ri):
        r3 = ri.reshape(N, 3).astype(LD)
        ref = np.einsum("nce,ne->nc", Dinv, r3).reshape(-1)
        mag = np.einsum("nce,ne->nc", np.abs(Dinv), np.abs(r3)).reshape(-1)
        _worst(np.abs(zi.astype(LD) - ref), 8 * U * mag, "block-Jacobi z = D^-1 r", i, ratios, "z")

    if jac:
        check_z_jacobi(0, tr["z"][0], r[0])
    for i in range(k):
        rec = i + 1
        pi, qi, zi = p[rec], q[rec], z_of(i)
        replaced = bool(f["replaced_mask"] >> i & 1)
        # ---- product ------------------------------------------------------------------------------------------------
        ref = row_dot(Hcg, pi)
        if replaced:
            hx = row_dot(H, x[rec])
            _worst(np.abs(qi.astype(LD) - hx), (nnz_row + 4) * U * row_dot(H, x[rec], True), "replacement product q = H x", i, ratios,
                   "replace")
        elif f["matfree"]:
            _worst(float(np.abs(qi.astype(LD) - ref).max()), 1e-12 * float(np.abs(ref).max()), "matrix-free product q = H p", i,
                   ratios, "product")
        else:
            _worst(np.abs(qi.astype(LD) - ref), (nnz_row + 4) * U * row_dot(Hcg, pi, True), "product q = H p", i, ratios, "product")
        # ---- direction ----------------------------------------------------------------------------------------------
        if i == 0:
            if not np.array_equal(pi, zi):
                j = int(np.argmax(pi != zi))
                raise TraceError("direction, iteration 0: p_0 differs from z_0 at entry %d (node row %d)" % (j, j // 3))
        else:
            beta = LD(rz_of(i)) / LD(rz_of(i - 1))
            t = beta * p[rec - 1].astype(LD)
            _worst(np.abs(pi.astype(LD) - (zi.astype(LD) + t)), 32 * U * (np.abs(zi) + np.abs(t).astype(np.float64)),
                   "direction p = z + beta p", i, ratios, "direction")
        # ---- update -------------------------------------------------------------------------------------------------
        alpha = LD(rz_of(i)) / LD(sums[rec, 2])
        t = alpha * pi.astype(LD)
        _worst(np.abs(x[rec].astype(LD) - (x[i].astype(LD) + t)), 32 * U * (np.abs(x[i]) + np.abs(t).astype(np.float64)),
               "update x += alpha p", i, ratios, "update")
        if replaced:
            _worst(np.abs(r[rec].astype(LD) - (b.astype(LD) - hx)), (nnz_row + 4) * U * (np.abs(b) + row_dot(H, x[rec], True)),
                   "residual replacement r = b - H x", i, ratios, "replace")
            d = b.astype(LD) - qi.astype(LD)
            _worst(np.abs(r[rec].astype(LD) - d), U * np.abs(d).astype(np.float64), "residual replacement r = b - q", i, ratios, "replace")
        else:
            t = alpha * qi.astype(LD)
            _worst(np.abs(r[rec].astype(LD) - (r[i].astype(LD) - t)), 32 * U * (np.abs(r[i]) + np.abs(t).astype(np.float64)),
                   "update r -= alpha q", i, ratios, "update")
        # ---- dots ---------------------------------------------------------------------------------------------------
        if replaced:  # q_i is gone: against p . (H p) of the working operator, with the product's own bound on top
            prod = pi.astype(LD) * ref
            slack = float((np.abs(pi) * (nnz_row + 4) * U * row_dot(Hcg, pi, True)).sum())
            _worst(abs(float(LD(sums[rec, 2]) - prod.sum())), (loops["pq"] + TAIL + 2) * U * float(np.abs(prod).sum()) + slack,
                   "p.q sum", i, ratios, "dot")
        else:
            _dot(ratios, "dot", "p.q sum", i, sums[rec, 2], pi, qi, loops["pq"] + TAIL)
        _dot(ratios, "dot", "r.r sum", i, sums[rec, 3], r[rec], r[rec], loops["rr"] + TAIL)
        _dot(ratios, "dot", "r.z sum", i, rz_of(i), r[i], zi, (loops["init"] if jac and i == 0 else loops["rz"]) + TAIL)
        if jac:  # the update kernel also left z and r.z of the new residual
            _dot(ratios, "dot", "r.z sum of the new residual", i, sums[rec, 1 - (i & 1)], r[rec], tr["z"][rec], loops["rz"] + TAIL)
            check_z_jacobi(i + 1, tr["z"][rec], r[rec])
        # ---- raw slots: their totals, and exact zeros beyond the grid that wrote them ---------------------------------------
        pq_grid = matfree_grid(N) if f["matfree"] else f["grid"]
        rz_grid = f["update_grid"] if jac else max(1, min(NPART, ceil_div(N, 32)))
        grids = {2: pq_grid, 3: f["update_grid"], (1 - (i & 1)) if jac else (i & 1): rz_grid}
        for a, g in grids.items():
            if np.any(slots[rec, a, g:] != 0.0):
                raise TraceError("slot array %d, iteration %d: a slot at or beyond the grid %d is not 0" % (a, i, g))
        for a in range(4):
            s = slots[rec, a].astype(LD)
            _worst(abs(float(LD(sums[rec, a]) - s.sum())), (2 + 6 + 16 + 2) * U * float(np.abs(s).sum()), "total of slot array %d" % a, i,
                   ratios, "slots")
    # ---- preconditioner output of the polynomial forms ------------------------------------------------------------------------
    if not jac and precond is not None:
        for i in range(k if z_records is None else min(k, z_records)):
            zr = precond(r[i])
            err = float(np.linalg.norm(z_of(i) - zr) / np.linalg.norm(zr))
            _worst(err, z_bound, "preconditioner z = M^-1 r", i, ratios, "z")
    return ratios


# ---- a plain PCG that writes the same records (tests/test_cg_np.py) ------------------------------------------------------------
def slot_sum(prod, grid):
    """a dot product through `grid` slots, as the kernels leave it: (slots [512], total)"""
    s = np.zeros(NPART)
    for g in range(grid):
        s[g] = prod[g::grid].sum()
    return s, float(s.sum())


FAULTS = ("q_misses_last_block", "q_row_doubled", "pq_slot_dropped", "beta_slots_swapped", "p_old_for_p_new",
          "last_row_left_stale", "float32_matrix_unreported")


def numpy_trace(H, b, k, lanes=32, fused=True, spmv32=False, replace_every=0, fault=None, fault_it=2, fault_row=None):
    """block-Jacobi PCG in fp64 from x = 0 for k iterations in the record layout of tlfea_newton_cg_trace.  fault: one of
    FAULTS, committed in iteration fault_it (on node row fault_row where it has a row) the way a wrong kernel would commit
    it -- everything after it is computed from the faulty value."""
    H = sp.csr_matrix(H)
    n = H.shape[0]
    N = n // 3
    Dinv = dinv_blocks(H).astype(np.float64)
    prec = lambda v: np.einsum("nce,ne->nc", Dinv, v.reshape(N, 3)).reshape(-1)
    as32 = spmv32 or fault == "float32_matrix_unreported"
    Hcg = sp.csr_matrix((H.data.astype(np.float32).astype(np.float64), H.indices, H.indptr), shape=H.shape) if as32 else H
    grid, ug = spmv_grid(N), slot_grid_256(N)
    fault_row = N - 1 if fault_row is None or fault == "last_row_left_stale" else fault_row
    form = dict(fused=int(fused), lanes=lanes, nt=0, tiled=1, xcd=0, grid=grid, graphs=0, spmv32=int(spmv32), replaced_mask=0,
                update=0, matfree=0, degree=1, precond=0, bits=64, block12=0, update_grid=ug, replace_lanes=lanes,
                replace_grid=grid, replace_xcd=0, xcd_mode=1)
    tr = dict(x=np.zeros((k + 1, n)), r=np.zeros((k + 1, n)), z=np.zeros((k + 1, n)), p=np.zeros((k + 1, n)),
              q=np.zeros((k + 1, n)), sums=np.zeros((k + 1, 4)), slots=np.zeros((k + 1, 5, NPART)), form=form)
    x, r = np.zeros(n), np.array(b, dtype=np.float64)
    z = prec(r)
    part = np.zeros((5, NPART))
    part[0], _ = slot_sum(r * z, NPART)
    part[4], _ = slot_sum(r * r, NPART)
    p = np.zeros(n)

    def record(j, p_, q_):
        tr["x"][j], tr["r"][j], tr["z"][j], tr["p"][j], tr["q"][j] = x, r, z, p_, q_
        tr["slots"][j] = part
        tr["sums"][j] = part[:4].sum(axis=1)

    record(0, 0.0, 0.0)
    for i in range(k):
        cur = i & 1
        rz_new, rz_old = part[cur].sum(), part[1 - cur].sum()
        hit = fault is not None and i == fault_it
        p_old, q_old = p, tr["q"][i]
        if i == 0:
            p = z.copy()
        else:
            p = z + (rz_old / rz_new if hit and fault == "beta_slots_swapped" else rz_new / rz_old) * p
        q = Hcg @ p
        rows = slice(3 * fault_row, 3 * fault_row + 3)
        if hit and fault == "q_misses_last_block":
            for c in range(3 * fault_row, 3 * fault_row + 3):
                last = slice(H.indptr[c + 1] - 3, H.indptr[c + 1])
                q[c] -= H.data[last] @ p[H.indices[last]]
        if hit and fault == "q_row_doubled":
            q[rows] *= 2.0
        if hit and fault == "last_row_left_stale":
            q[rows] = q_old[rows]
        part[2], pq = slot_sum(p * q, grid)
        if hit and fault == "pq_slot_dropped":
            pq -= part[2][grid // 2]
            part[2][grid // 2] = 0.0
        alpha = rz_new / pq
        x = x + alpha * (p_old if hit and fault == "p_old_for_p_new" else p)
        if replace_every and (i + 1) % replace_every == 0:
            q = H @ x                      # the replacement's product reuses the q buffer
            r = b - q
            form["replaced_mask"] |= 1 << i
        else:
            r = r - alpha * q
        z = prec(r)
        part[1 - cur], _ = slot_sum(r * z, ug)
        part[3], _ = slot_sum(r * r, ug)
        record(i + 1, p, q)
    return tr
