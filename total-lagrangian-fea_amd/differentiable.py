"""Differentiable implicit step of a T10 body or an ANCF beam / shell body (DESIGN 3j'): torch.autograd over
SyncedNewtonSolver.Solve().

One step with max_outer = 1 maps the state (x, v, lambda) and the inputs f_ext, constraint targets, body acceleration
and material parameters to the next state.  ImplicitStep runs the engine's own forward step and, in backward, the
adjoint step on the device (tlfea_newton_adjoint_step_device): one linear solve with the step's Hessian per step.

Tensors are float64 on the CPU (the engine's setters take host arrays); backward moves the cotangents to the GPU and
calls the device form.  The materials tensor is [n_mat, P + 1] in the model's natural parameters -- SVK (lambda, mu, rho0),
Mooney-Rivlin (mu10, mu01, kappa, rho0); lame_from_E_nu / E_nu_from_lame are written in torch, so the chain rule to
(E, nu) is autograd's.  Densities enter the mass matrix: a forward whose densities differ from the ones the mass matrix
was assembled with runs CalcMassMatrix again (and so does a backward that has to go back to them).

The optional trailing `reference` tensor [N, 3] is the reference geometry X of all ten nodes of every element:
a forward whose reference differs from the geometry last applied calls SetReferencePositions (and so does a backward that
has to go back), and backward returns its cotangent.  straight_sided() places the mid-edge nodes at the means of their
vertices in torch, so a vertex-only parametrisation differentiates through autograd.  With a reference that requires a
gradient, obstacles and face tractions are refused as well.

An ANCF data object (GPU_ANCF3243_Data, GPU_ANCF3443_Data) dispatches to the ANCF entry points by its class: x and v are
[n_coef, 3] over all coefficient vectors, targets [n_fixed, 3] those of the fixed coefficients (or the CSR right-hand side),
materials [1, P + 1] (one material per object), gravity acts on the position coefficients.  A density change reruns
CalcMassMatrix, on the host for these kinds.  `reference` is refused: ANCF shape sensitivities are not built.

Not differentiated (refused by the adjoint step): damping, friction, follower pressure, a partitioned mesh, steps with more
than one outer iteration; on ANCF bodies also the reference geometry and the cross-section.
"""
import numpy as np
import torch

from .binding import AdjointInC, AdjointOutC, TlfeaError
from .elements import ElementMaterial, _GPU_ANCF_Data


def lame_from_E_nu(E, nu):
    """(lambda, mu) from Young's modulus and Poisson's ratio (torch tensors or floats)"""
    return E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu)), E / (2.0 * (1.0 + nu))


def E_nu_from_lame(lam, mu):
    """(E, nu) from the Lame parameters"""
    return mu * (3.0 * lam + 2.0 * mu) / (lam + mu), lam / (2.0 * (lam + mu))


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def _is_ancf(data):
    return isinstance(data, _GPU_ANCF_Data)


def _material_shape(data):
    return data.ANCFMaterialSensitivityShape() if _is_ancf(data) else data.MaterialSensitivityShape()


def _fixed_targets(data, t):
    """full target arrays from the [n_fixed, 3] rows of the fixed nodes / coefficients (targets of free ones are never read)"""
    full = np.array(data._X0, dtype=np.float64)
    if t is not None:
        full[data.fixed_nodes] = t.reshape(-1, 3)
    return full


def _apply_inputs(solver, data, f_ext, targets, gravity, materials):
    """Write one step's differentiable inputs into the objects (None = leave what is set)."""
    if materials is not None:
        m = _np(materials)
        n_mat, slots = _material_shape(data)
        if m.shape != (n_mat, slots):
            raise ValueError(f"materials must be [{n_mat}, {slots}] for the model and table set, got {tuple(m.shape)}")
        ids = None if _is_ancf(data) else data.GetElementMaterialIds()
        if slots == 3:
            En = [E_nu_from_lame(r[0], r[1]) for r in m]
            mats = [ElementMaterial(E=e, nu=nu, rho0=r[2]) for (e, nu), r in zip(En, m)]
        else:
            mats = [ElementMaterial(mu10=r[0], mu01=r[1], kappa=r[2], rho0=r[3]) for r in m]
        if ids is not None:
            data.SetElementMaterials(ids, mats, model="svk" if slots == 3 else "mooney_rivlin")
        elif slots == 3:
            data.SetSVK(mats[0].E, mats[0].nu)
            data.SetDensity(mats[0].rho0)
        else:
            data.SetMooneyRivlin(mats[0].mu10, mats[0].mu01, mats[0].kappa)
            data.SetDensity(mats[0].rho0)
        rho = m[:, -1].copy()
        if getattr(data, "_mass_rho", None) is None or not np.array_equal(data._mass_rho, rho):
            moved = _is_ancf(data) and getattr(data, "_targets_applied", None) is not None
            if moved:  # an ANCF object keeps its targets where its reference coefficients are, and the mass rule reads those
                X0 = data._X0
                data.UpdateConstraintTargets(X0[:, 0], X0[:, 1], X0[:, 2])
            data.CalcMassMatrix()
            if moved:
                full = data._targets_applied
                data.UpdateConstraintTargets(full[:, 0], full[:, 1], full[:, 2])
            data._mass_rho = rho
    if gravity is not None:
        data.SetGravity(_np(gravity).reshape(3))
    if f_ext is not None:
        data.SetExternalForce(_np(f_ext).reshape(-1))
    if targets is not None:
        t = _np(targets)
        if data.GetConstraintMode() == 2:
            data.UpdateLinearConstraintRHS(t.reshape(-1))
        else:
            full = _fixed_targets(data, t)
            data.UpdateConstraintTargets(full[:, 0], full[:, 1], full[:, 2])
            data._targets_applied = full


_EDGES = ((0, 1), (1, 2), (0, 2), (0, 3), (1, 3), (2, 3))  # mid-edge node 4 + k lies between these vertices


def straight_sided(Xv, conn):
    """All-node coordinates [N, 3] of a straight-sided mesh from Xv [N, 3], of which only the vertex rows are read: every
    mid-edge node is the mean of its two vertices.  conn [E, 10] (numpy or tensor of node ids)."""
    c = np.asarray(conn.cpu() if torch.is_tensor(conn) else conn).astype(np.int64)
    mid = np.concatenate([c[:, 4 + k] for k in range(6)])
    va = np.concatenate([c[:, i] for i, _ in _EDGES])
    vb = np.concatenate([c[:, j] for _, j in _EDGES])
    mid, first = np.unique(mid, return_index=True)  # an edge shared by several elements has the same two vertices in all
    mid, va, vb = (torch.as_tensor(a, device=Xv.device) for a in (mid, va[first], vb[first]))
    X = Xv.clone()
    X[mid] = 0.5 * (Xv[va] + Xv[vb])
    return X


def _apply_reference(data, reference):
    """Move the object's reference geometry where it differs from the one last applied (None = leave it)."""
    if reference is None:
        return
    R = _np(reference).reshape(-1, 3)
    if not np.array_equal(np.asarray(data._X0), R):
        data.SetReferencePositions(R)


class ImplicitStep(torch.autograd.Function):
    """(x, v, lambda)_new = ImplicitStep.apply(solver, data, x, v, lam, f_ext, targets, gravity, materials[, reference]).

    x, v [N, 3] (N = n_coef), lam [n_constraints]; f_ext [N, 3]; targets [n_fixed, 3] (positions of data.fixed_nodes, in their order)
    or the right-hand side [n_constraints] of CSR constraints; gravity [3]; materials [n_mat, P + 1].  Any of the last four
    may be None: the objects keep what is set and no gradient flows.  reference [N, 3] (optional): the reference geometry.
    The solver's parameters must have max_outer = 1."""

    @staticmethod
    def forward(ctx, solver, data, x, v, lam, f_ext, targets, gravity, materials, reference=None):
        ancf = _is_ancf(data)
        if ancf and reference is not None:
            raise ValueError("ImplicitStep: `reference` is not available on an ANCF object -- shape and cross-section "
                             "sensitivities of the ANCF kinds are not built (DESIGN 9)")
        _apply_reference(data, reference)
        _apply_inputs(solver, data, f_ext, targets, gravity, materials)
        xn, vn = _np(x).reshape(-1, 3), _np(v).reshape(-1)
        data.UpdatePositions(xn[:, 0], xn[:, 1], xn[:, 2])
        solver.SetVelocity(vn, vn)  # the step starts from v_prev = v: Solve() ends every step that way
        if solver.n_constraints:
            solver.SetLambda(_np(lam).reshape(-1))
        solver.Solve()
        # a step the adjoint would refuse is refused here, where the cause is
        solver.ANCFAdjointReady() if ancf else solver.AdjointReady()
        x1 = np.stack(data.RetrievePositionToCPU(), axis=1)
        v1 = solver.RetrieveVelocityToCPU().reshape(-1, 3)
        lam1 = solver.RetrieveLambdaToCPU()
        ctx.solver, ctx.data = solver, data
        ctx.inputs = (f_ext, targets, gravity, materials)
        ctx.reference = reference
        ctx.state = (x1, v1, lam1, vn.copy())
        ctx.shapes = (x.shape, v.shape, lam.shape)
        return (torch.tensor(x1).reshape(x.shape), torch.tensor(v1).reshape(v.shape), torch.tensor(lam1).reshape(lam.shape))

    @staticmethod
    def backward(ctx, gx, gv, glam):
        solver, data = ctx.solver, ctx.data
        f_ext, targets, gravity, materials = ctx.inputs
        x1, v1, lam1, v0 = ctx.state
        # that step's converged state and inputs again (H depends on x, the reference, the materials and the time step)
        reference = ctx.reference
        _apply_reference(data, reference)
        _apply_inputs(solver, data, None, None, gravity, materials)
        data.UpdatePositions(x1[:, 0], x1[:, 1], x1[:, 2])
        solver.SetVelocity(v1.reshape(-1), v1.reshape(-1))
        if solver.n_constraints:
            solver.SetLambda(lam1)
        dev = torch.device("cuda")
        N, nc = data.n_coef, solver.n_constraints
        n_mat, slots = _material_shape(data)

        def up(t):
            return None if t is None else t.detach().to(dev, torch.float64).contiguous().reshape(-1)
        ins = [up(gx), up(gv), up(glam) if nc else None, torch.from_numpy(v0).to(dev)]
        want = {"f_ext": f_ext is not None and ctx.needs_input_grad[5], "t": targets is not None and ctx.needs_input_grad[6],
                "a": gravity is not None and ctx.needs_input_grad[7], "m": materials is not None and ctx.needs_input_grad[8]}
        z = lambda k: torch.zeros(k, dtype=torch.float64, device=dev)  # noqa: E731
        outs = [z(3 * N), z(3 * N), z(3 * N), z(nc) if nc else None, z(nc) if nc and want["t"] else None,
                z(3) if want["a"] else None, z(n_mat * slots) if want["m"] else None, None]
        want_X = reference is not None and len(ctx.needs_input_grad) > 9 and ctx.needs_input_grad[9]
        X_bar = z(3 * N) if want_X else None
        torch.cuda.synchronize()
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        cin, cout = AdjointInC(*[ptr(t) for t in ins]), AdjointOutC(*[ptr(t) for t in outs])
        if _is_ancf(data):
            solver.ANCFAdjointStepDevice(cin, cout)
        else:
            solver.AdjointStepDevice(cin, cout, ptr(X_bar))
        sx, sv, sl = ctx.shapes
        back = lambda t, shape: None if t is None else t.cpu().reshape(shape)  # noqa: E731
        return (None, None, back(outs[2], sx), back(outs[1], sv), back(outs[3], sl) if nc else torch.zeros(sl, dtype=torch.float64),
                back(outs[0], f_ext.shape) if want["f_ext"] else None,
                back(outs[4], targets.shape) if want["t"] and nc else None,
                back(outs[5], gravity.shape) if want["a"] else None,
                back(outs[6], materials.shape) if want["m"] else None,
                back(X_bar, reference.shape) if want_X else None)  # a nine-argument call: torch drops the trailing None


def rollout(solver, data, state, n_steps, f_ext=None, targets=None, gravity=None, materials=None, reference=None):
    """n_steps chained ImplicitStep calls from state = (x, v, lam); the inputs are the same tensors in every step (their
    gradients add up).  A rollout that starts at x_0 = reference gets that path from autograd.  -> the final (x, v, lam)."""
    x, v, lam = state
    for _ in range(int(n_steps)):
        if reference is None:
            x, v, lam = ImplicitStep.apply(solver, data, x, v, lam, f_ext, targets, gravity, materials)
        else:
            x, v, lam = ImplicitStep.apply(solver, data, x, v, lam, f_ext, targets, gravity, materials, reference)
    return x, v, lam


__all__ = ["ImplicitStep", "rollout", "straight_sided", "lame_from_E_nu", "E_nu_from_lame", "TlfeaError"]
