"""NumPy restatement of the stress recovery: Cauchy stress, strain-energy density, viscous power, element and
nodal means and the five totals, from F per (element, point), the material, det J, the weights and the connectivity."""
import numpy as np

VOIGT = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0))  # stored order xx yy zz xy yz zx


def lame(m):
    return m["E"] * m["nu"] / ((1 + m["nu"]) * (1 - 2 * m["nu"])), m["E"] / (2 * (1 + m["nu"]))


def elastic_P(F, m):
    """First Piola-Kirchhoff stress of helpers.MATERIALS-style records, F [..., 3, 3]."""
    C = np.swapaxes(F, -1, -2) @ F
    if m["kind"] == "svk":
        lam, mu = lame(m)
        E = 0.5 * (C - np.eye(3))
        return F @ (lam * np.trace(E, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) + 2 * mu * E)
    J = np.linalg.det(F)[..., None, None]
    G = np.swapaxes(np.linalg.inv(F), -1, -2)
    I1 = np.trace(C, axis1=-2, axis2=-1)[..., None, None]
    I2 = 0.5 * (I1 ** 2 - np.trace(C @ C, axis1=-2, axis2=-1)[..., None, None])
    return (2 * m["mu10"] * J ** (-2 / 3) * (F - I1 / 3 * G) + 2 * m["mu01"] * J ** (-4 / 3) * (I1 * F - F @ C - 2 * I2 / 3 * G)
            + m["kappa"] * (J - 1) * J * G)


def viscous_P(F, Fd, m):
    """Kelvin-Voigt part F (2 eta Edot + lamd tr Edot I), Edot = sym(Fdot^T F)."""
    Ed = 0.5 * (np.swapaxes(Fd, -1, -2) @ F + np.swapaxes(F, -1, -2) @ Fd)
    return F @ (2 * m["eta"] * Ed + m["lamd"] * np.trace(Ed, axis1=-2, axis2=-1)[..., None, None] * np.eye(3))


def psi(F, m):
    """Elastic strain-energy density per reference volume."""
    C = np.swapaxes(F, -1, -2) @ F
    if m["kind"] == "svk":
        lam, mu = lame(m)
        E = 0.5 * (C - np.eye(3))
        return 0.5 * lam * np.trace(E, axis1=-2, axis2=-1) ** 2 + mu * np.sum(E * E, axis=(-2, -1))
    J = np.linalg.det(F)
    I1 = np.trace(C, axis1=-2, axis2=-1)
    I2 = 0.5 * (I1 ** 2 - np.trace(C @ C, axis1=-2, axis2=-1))
    return m["mu10"] * (J ** (-2 / 3) * I1 - 3) + m["mu01"] * (J ** (-4 / 3) * I2 - 3) + 0.5 * m["kappa"] * (J - 1) ** 2


def voigt(S):
    return np.stack([S[..., i, j] for i, j in VOIGT], axis=-1)


def tensor(s6):
    S = np.zeros(s6.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate(VOIGT):
        S[..., i, j] = S[..., j, i] = s6[..., k]
    return S


def von_mises(s):
    return np.sqrt(0.5 * ((s[..., 0] - s[..., 1]) ** 2 + (s[..., 1] - s[..., 2]) ** 2 + (s[..., 2] - s[..., 0]) ** 2)
                   + 3 * (s[..., 3] ** 2 + s[..., 4] ** 2 + s[..., 5] ** 2))


def deformation(x, conn, gradN):
    """F [E, Q, 3, 3] = sum_a x_a (x) grad N_a; x [N, 3], gradN [E, Q, 10, 3]."""
    return np.einsum("eai,eqaj->eqij", x[conn], gradN)


def recover(F, m, detJ, qw, conn, n_nodes, Fdot=None, materials=None):
    """Every field and total.  m: one material record, or (with materials = list of records) ignored in favour of
    materials[k] for the elements of mask k given as m = element ids.  Returns a dict."""
    if materials is None:
        P = elastic_P(F, m)
        W = psi(F, m)
        Pv = viscous_P(F, Fdot, m) if Fdot is not None and (m["eta"] != 0 or m["lamd"] != 0) else np.zeros_like(F)
    else:
        ids = np.asarray(m)
        P, W, Pv = np.zeros_like(F), np.zeros(F.shape[:2]), np.zeros_like(F)
        for k, mk in enumerate(materials):
            sel = ids == k
            P[sel], W[sel] = elastic_P(F[sel], mk), psi(F[sel], mk)
            if Fdot is not None and (mk["eta"] != 0 or mk["lamd"] != 0):
                Pv[sel] = viscous_P(F[sel], Fdot[sel], mk)
    J = np.linalg.det(F)
    sig_full = (P + Pv) @ np.swapaxes(F, -1, -2) / J[..., None, None]
    sig = voigt(sig_full)
    power = np.sum(Pv * Fdot, axis=(-2, -1)) if Fdot is not None else np.zeros(F.shape[:2])
    dV = detJ * np.asarray(qw)[None, :]
    Ve = dV.sum(axis=1)
    wq = dV / Ve[:, None]
    es = np.einsum("eq,eqc->ec", wq, sig)
    num = np.zeros((n_nodes, 6))
    den = np.zeros(n_nodes)
    for a in range(conn.shape[1]):
        np.add.at(num, conn[:, a], Ve[:, None] * es)
        np.add.at(den, conn[:, a], Ve)
    ns = num / np.where(den > 0, den, 1.0)[:, None]
    return dict(point_sigma=sig, point_sigma_full=sig_full, P=P + Pv, J=J, elem_sigma=es, elem_von_mises=von_mises(es),
                elem_psi=(wq * W).sum(axis=1), elem_J=(wq * J).sum(axis=1), elem_volume=Ve, nodal_sigma=ns,
                nodal_von_mises=von_mises(ns), strain_energy=float((W * dV).sum()), viscous_power=float((power * dV).sum()),
                reference_volume=float(dV.sum()), current_volume=float((J * dV).sum()))


def kinetic_energy(off, col, val, v):
    """1/2 v^T M v with M (scalar per node pair) in CSR; v [3N]."""
    v3 = np.asarray(v).reshape(-1, 3)
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return 0.5 * float(np.sum(val * np.einsum("ki,ki->k", v3[rows], v3[col])))
