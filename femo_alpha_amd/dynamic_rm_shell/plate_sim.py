"""``PlateSim``: transient (midpoint / Newmark) RM shell on one MI355X.

Interface of femo_alpha/dynamic_rm_shell/plate_sim.py:60-361 (constructor, ``update_t``,
``update_f_history``, ``solve_dynamic_problem``, ``assembleStrainEnergy``) plus the adjoint pieces the dynamic
operators need.  Time discretisation as in the reference (:131-140):

    w_mid = (w_old + w)/2,  wdot = 2/dt (w - w_old) - wdot_old,  wddot = (wdot - wdot_old)/dt
    R_i   = M wddot_i + K w_mid,i - F_i = 0     (force taken at the new level, :312-316)

so every step solves  (2/dt^2 M + K/2) w_i = F_i + M (2/dt^2 w_{i-1} + 2/dt wdot_{i-1}) - K/2 w_{i-1}.

PARITY UNPINNED for this path: the energy / inertia forms of the reference come from ``shell_analysis_fenicsx``,
which is neither vendored nor version-pinned (plate_sim.py:17,193-201); the vendored sibling is used as the
nearest text: elastic energy of linear_shell_model.py:275-306 at uhat = 0, inertia rho t (u.v + h_K^2 theta.eta)
(:335-348), membrane/bending/shear on the degree-``quad_deg`` rule, drilling and inertia on the full rule.

The operator is linear and constant over the march, so it is factorised once per thickness (the reference
re-assembles and re-factorises it every step, nonlinear_utils.py:210-233) and each step is one preconditioned
solve; the adjoint is the O(T) two-vector recursion instead of the reference's O(T^2) history sums
(state_operation_dynamic.py:606-702).  The march, the backward sweep and the per-level gradient products run inside
libfemo_hip (``femo_newmark_*``, include/femo_hip.h) with the histories resident in HBM: one call per march, the pressure
history uploaded once.  History layout at the boundary: (fe_dofs, time_levels), flattened
column-major by the operators (dynamic_rm_shell/utils.py:9-16).
"""
from __future__ import annotations

import numpy as np

from ..backend import ShellContext


class PlateSim:
    def __init__(self, mesh, E, nu, rho, dt, Nsteps, element_wise_thickness=False, custom_bc_func=None,
                 add_self_weight=False, g_factor=None, quad_deg=3, comm=None, device=0, leaf_size=None, rtol=1e-8, tail_max=None):
        import torch
        self.torch = torch
        self.mesh, self.E, self.nu, self.rho, self.dt = mesh, E, nu, rho, dt
        self.Nsteps, self.time_levels = Nsteps, Nsteps + 1
        self.nn, self.nel = mesh.nn, mesh.nel
        self.element_wise_thickness = element_wise_thickness
        self.add_self_weight, self.g_factor, self.quad_deg = add_self_weight, g_factor, quad_deg
        # self weight f_d = (0, 0, rho t g) (plate_sim.py:203-214): with nodal thickness it rides on the nodal pressure field;
        # with element-wise thickness it is a cell-wise constant pressure, applied as its consistent P2 nodal loads
        self._sw_weights = mesh.p2_integrals() if (add_self_weight and element_wise_thickness) else None
        ctx = self.ctx = ShellContext(mesh, element_wise_material=element_wise_thickness, device=device)
        ctx.set_field("E", [E]); ctx.set_field("nu", [nu]); ctx.set_field("density", [rho])
        marker = custom_bc_func if custom_bc_func is not None else (lambda x: np.isclose(x[0], 0.0, atol=1e-6))
        self.bc_dofs = mesh.locate_dofs_geometrical(marker)            # plate_sim.py:34-58
        ctx.set_strong_dofs(self.bc_dofs)
        npts = (quad_deg + 2) // 2                                       # Gauss points per direction for that degree
        if mesh.is_quad and npts < 4:
            ctx.set_strain_quadrature(npts)
        # tail_max: the tail-delay pass of the symbolic analysis (None: the context's default, on; 0: off)
        ctx.enable_frontal(leaf_size, **({} if tail_max is None else dict(tail_max=tail_max)))
        # The reference solves every step with ONE sparse LU solve (solveNonlinear_mod: a single Newton iteration,
        # nonlinear_utils.py:220-229).  Here the preconditioner is the exact Cholesky factor of the step operator: its first
        # application is that direct solve (relative residual 6e-9 at 508 k DOF, the history within 7e-10 of the fully converged
        # one, scripts/r3_dyn_probe.py), a second one drives the residual to 1e-18.  rtol = 1e-8 stops after the first, as the
        # reference does; rtol = 1e-11 buys the refinement step for 40 % more time per step.
        self.rtol = float(rtol)
        ctx.set_solver(preconditioner=2, rtol=rtol, maxit=50, check_every=1)
        self.a, self.b = 2.0 / dt ** 2, 2.0 / dt
        ctx.set_operator(0.5, self.a)
        self.fe_dofs = ctx.ndof
        self.num_var = ctx.field_size("thickness")
        self.f_history = np.zeros((self.time_levels, 3 * mesh.nn))
        self.t = np.full(self.num_var, 1e-3)
        self.opt_iter = 0
        self.W = None                      # device history, (time_levels, fe_dofs)
        # tip displacement history (plate_sim.py:22-23, 107, 116-117, 154-156, 323-328): uz at x_tip, refreshed by every march
        self.x_tip, self.cell_tip = None, None
        self._tip = None                   # (dofs, weights) of the probe, False where the default point lies in no cell
        self.tip_disp_history = np.zeros(self.time_levels)
        self.solve_info = []
        self._v = {n: ctx.vec_tensor(n) for n in ("state", "adjoint", "r", "z", "p", "Ap", "b")}

    # ------------------------------------------------------------------ inputs
    def update_t(self, t_array):
        self.t = np.asarray(t_array, dtype=np.float64).ravel().copy()
        self.ctx.set_field("thickness", self.t)

    def update_f_history(self, f_history_array):
        self.f_history = np.asarray(f_history_array, dtype=np.float64).reshape(-1, 3 * self.nn)

    def update_nsteps(self, Nsteps):
        self.Nsteps, self.time_levels = Nsteps, Nsteps + 1
        self._nm_ready = False
        # the next set-up re-allocates the resident histories: the zero-copy views of the old ones must not outlive them
        self.W = None
        self.Lam = None
        self.tip_disp_history = np.zeros(self.time_levels)

    def _gravity(self):
        return (-1.0 if self.g_factor is None else self.g_factor) * 9.81

    def _force_history(self):
        """(time_levels, 3 nn) pressure history as the library marches it; self weight f_d = (0, 0, rho t g) rides on it when the
        thickness is nodal (plate_sim.py:204-211)."""
        k = np.minimum(np.arange(self.time_levels), self.f_history.shape[0] - 1)
        F = self.f_history[k].reshape(self.time_levels, -1, 3).copy()
        if self.add_self_weight and self._sw_weights is None:
            F[:, :, 2] += (self.rho * self.t * self._gravity())[None, :]
        return F.reshape(self.time_levels, -1)

    def _force_at(self, i):
        return self._force_history()[i].reshape(-1, 3)

    def _self_weight_load(self):
        """Self-weight load vector for element-wise thickness: F[3 p + 2] += rho t_e g int N2_a dS."""
        F = np.zeros(self.fe_dofs)
        np.add.at(F, 3 * self.mesh.cell_p2.ravel() + 2, (self._sw_weights * (self.rho * self._gravity() * self.t)[:, None]).ravel())
        F[self.bc_dofs] = 0.0
        return F

    # ------------------------------------------------------------------ forward march
    def _sync(self):
        self.torch.cuda.synchronize()

    def _newmark(self):
        if not getattr(self, "_nm_ready", False):
            self.ctx.newmark_setup(self.time_levels, self.dt)
            self._nm_ready = True

    def solve_dynamic_problem(self, residual=None, saving_outputs=False, PATH=None, timing=False, reassemble_every_step=False):
        """March from zero initial conditions; returns the (fe_dofs, time_levels) history.

        ``reassemble_every_step``: rebuild and re-factorise the step operator before every solve, as the reference does
        (``solveNonlinear_mod`` assembles the Jacobian and runs a fresh LU per step, nonlinear_utils.py:210-233 from
        plate_sim.py:319).  The operator does not change along the march, so the default factorises once per thickness;
        the flag exists so that BASELINE config 5 can be timed as written ("re-assembly per step")."""
        ctx = self.ctx
        self._newmark()
        ctx.newmark_set_forces(self._force_history())
        ctx.newmark_set_constant_load(self._self_weight_load() if self._sw_weights is not None else None)
        self.solve_info = ctx.newmark_march(self.Nsteps, reassemble_every_step)
        self.W = ctx.newmark_tensor(0)                 # device history, (time_levels, fe_dofs), zero-copy
        self.tip_disp_history = self.tip_displacement_history()
        return ctx.newmark_history(0).T.copy(order="F")

    def energy_audit(self):
        """Discrete energy balance of the last march.  The midpoint rule with the force at the new level satisfies
            (T_i + U_i) - (T_{i-1} + U_{i-1}) = F_i . (w_i - w_{i-1})        exactly,
        T = 1/2 wdot^T M wdot, U = 1/2 w^T K w (multiply the step equation by w_i - w_{i-1} = dt (wdot_i + wdot_{i-1}) / 2).
        Returns (U, T, work) as arrays over the time levels, evaluated by the matrix-free operator on the device history --
        a size-independent check of the whole step (operator, inertia, solve, Dirichlet rows)."""
        ctx, v, torch = self.ctx, self._v, self.torch
        W = self.W
        U, T, work = np.zeros(self.time_levels), np.zeros(self.time_levels), np.zeros(self.time_levels)
        wdot = torch.zeros_like(v["state"])
        FH = self._force_history()
        for i in range(1, self.time_levels):
            wdot = self.b * (W[i] - W[i - 1]) - wdot
            v["p"].copy_(W[i]); v["adjoint"].copy_(wdot)
            self._sync()
            ctx.op_apply_vec2("p", "z", 1.0, 0.0, False)                # K w_i
            ctx.op_apply_vec2("adjoint", "Ap", 0.0, 1.0, False)         # M wdot_i
            ctx.set_field("F_solid", FH[i])
            ctx.load_vec("b")
            U[i] = 0.5 * float(torch.dot(W[i], v["z"]))
            T[i] = 0.5 * float(torch.dot(wdot, v["Ap"]))
            work[i] = float(torch.dot(v["b"], W[i] - W[i - 1]))
        return U, T, work

    # ------------------------------------------------------------------ post-processing the gust examples call
    def _level_state(self, level):
        if level is not None:
            self.ctx.set_state(self.W[level].cpu().numpy())

    def _stress_settings(self, m, rho, alpha, regularization):
        """m, rho, alpha (None: the area of the degree-4 measure) and the regularisation 0.5e3 int t^rho dx (plate_sim.py:438-441)
        into the context; alpha and the coefficient are sent only when they change."""
        self.ctx.set_stress_params(m, rho)
        alpha = None if alpha is None else float(alpha)
        if alpha != getattr(self, "_stress_alpha", None):
            self.ctx.set_stress_alpha(alpha)
            self._stress_alpha = alpha
        reg = 0.5e3 if regularization else 0.0
        if reg != getattr(self, "_stress_reg", 0.0):
            self.ctx.set_option("stress_regularization", reg)
            self._stress_reg = reg

    def pnorm_stress(self, m=1e-6, rho=100, alpha=None, regularization=False, level=None):
        """1/alpha [int (m vm_top)^rho dx (+ 0.5e3 int t^rho dx)] over the degree-4 measure (plate_sim.py:427-444) for the state of
        time level ``level`` (default: the state the context holds, i.e. the last level solved -- the reference's ``self.w``)."""
        self._level_state(level)
        self._stress_settings(m, rho, alpha, regularization)
        return self.ctx.functional("pnorm_stress")

    # ------------------------------------------------------------------ space-time stress aggregate (femo_newmark_stress_history*)
    def _history_arg(self, W):
        """None (the history of the last march, read in place on the device) or a (fe_dofs, time_levels) history as level-major rows."""
        if W is None:
            self._newmark()
            return None
        W = np.asarray(W, dtype=np.float64).reshape(self.fe_dofs, self.time_levels)
        return np.ascontiguousarray(W.T)

    def pnorm_stress_history(self, m=1e-6, rho=100, alpha=None, regularization=False, per_level=False, W=None):
        """S = sum over the time levels of pnorm_stress(level=i) (plate_sim.py:427-449), in one pass over the history; the max-stress
        estimate follows as AggregatedStressModel(m, rho).evaluate(S).  ``per_level``: the T values P_i instead.  ``W``: a
        (fe_dofs, time_levels) history (None: the last march's).  A P_i or S that overflows is an error (lower m)."""
        self._stress_settings(m, rho, alpha, regularization)
        S, P = self.ctx.newmark_stress_history(self.time_levels, self._history_arg(W))
        return P if per_level else S

    def pnorm_stress_history_partials(self, m=1e-6, rho=100, alpha=None, regularization=False, W=None):
        """(dS/dt, dS/dW) of ``pnorm_stress_history``; dS/dW in the boundary layout (fe_dofs, time_levels)."""
        self._stress_settings(m, rho, alpha, regularization)
        g, G = self.ctx.newmark_stress_history_grad(self.time_levels, self._history_arg(W))
        return g, G.T.copy(order="F")

    def pnorm_stress_history_total_gradient(self, m=1e-6, rho=100, alpha=None, regularization=False):
        """(dS/dt, dS/dF_history) through the transient adjoint, for the history of the last march.  The history gradient seeds the
        adjoint on the device (femo_newmark_adjoint_seeded), the residual products follow (self weight as residual_T_products
        treats it): dS/dt = dS/dt|_W - sum_i (dR_i/dt)^T lam_i, dS/dF = -[(dR_i/df)^T lam_i]_i, (time_levels, 3 nn)."""
        self._newmark()
        self._stress_settings(m, rho, alpha, regularization)
        T = self.time_levels
        g_part, _ = self.ctx.newmark_stress_history_grad(T, None, want_G=False, seed_adjoint=True)
        self.ctx.newmark_adjoint_seeded(T)
        self.Lam = self.ctx.newmark_tensor(2)
        g_t, dF = self.residual_T_products()
        return g_part - g_t, -dF

    # ------------------------------------------------------------------ tip displacement history
    DEFAULT_X_TIP = (10.0, 0.0, 0.0)       # extractTipDispDolfinx's default point (plate_sim.py:22)

    def set_up_tip_dofs(self, x_tip, cell_tip=None):
        """The point whose z displacement ``tip_disp_history`` records (plate_sim.py:154-156).  ``cell_tip`` is a cell index of the
        ShellMesh given to this PlateSim -- NOT the reference's dolfinx-internal index, which no other mesh shares; None locates the
        cell holding x_tip (ShellMesh.point_evaluation; an error if there is none)."""
        self._tip = self.mesh.point_evaluation(x_tip, cell=cell_tip, component=2)
        self.x_tip, self.cell_tip = x_tip, cell_tip

    def _tip_probe(self):
        if self._tip is None:
            if self.x_tip is not None:
                self._tip = self.mesh.point_evaluation(self.x_tip, cell=self.cell_tip, component=2)
            else:                         # the reference's default point, located; a mesh without it records zeros
                cell = self.mesh.locate(self.DEFAULT_X_TIP)
                self._tip = False if cell is None else self.mesh.point_evaluation(self.DEFAULT_X_TIP, cell=cell, component=2)
        return self._tip

    def tip_displacement_history(self, W=None):
        """uz at the tip point for every time level (time_levels,): a gather of the cell's npc uz columns of the history and a dot with
        the basis weights at the point -- on the device for the history of the last march (W = None), on the host for a given
        (fe_dofs, time_levels) W.  Zeros if no tip was set up and the default point lies in no cell."""
        probe = self._tip_probe()
        if probe is False:
            return np.zeros(self.time_levels)
        dofs, weights = probe
        if W is not None:
            return weights @ np.asarray(W, dtype=np.float64).reshape(self.fe_dofs, self.time_levels)[dofs, :]
        torch = self.torch
        dev = self.W.device
        idx = torch.as_tensor(dofs, dtype=torch.long, device=dev)
        return (self.W[:, idx] @ torch.as_tensor(weights, dtype=torch.float64, device=dev)).cpu().numpy()

    # ------------------------------------------------------------------ max-displacement aggregate (femo_newmark_disp_aggregate*)
    def max_displacement_history(self, rho, scaler=1.0, components="all", per_level=False, W=None):
        """M = csdl.maximum(csdl.absolute(scaler * W), rho) / scaler over the whole space-time history (ex_lpc_gust_response_opt.py:
        457-459, 770-772), as the KS aggregate of include/femo_hip.h, in one pass over the history.  components: "all" (every entry,
        rotations included) or "translations" (the mid-surface displacement).  ``per_level``: the T values M_i of each level alone.
        ``W``: a (fe_dofs, time_levels) history (None: the last march's, read in place)."""
        M, P = self.ctx.newmark_disp_aggregate(self.time_levels, rho, scaler, components, self._history_arg(W))
        return P if per_level else M

    def max_displacement_history_partials(self, rho, scaler=1.0, components="all", W=None):
        """dM/dW of ``max_displacement_history`` in the boundary layout (fe_dofs, time_levels); the thickness does not enter M."""
        _, G = self.ctx.newmark_disp_aggregate_grad(self.time_levels, rho, scaler, components, self._history_arg(W))
        return G.T.copy(order="F")

    def max_displacement_history_total_gradient(self, rho, scaler=1.0, components="all"):
        """(dM/dt, dM/dF_history) through the transient adjoint, for the history of the last march: dM/dW seeds the adjoint on the
        device (femo_newmark_adjoint_seeded), the residual products follow: dM/dt = -sum_i (dR_i/dt)^T lam_i,
        dM/dF = -[(dR_i/df)^T lam_i]_i, (time_levels, 3 nn)."""
        self._newmark()
        T = self.time_levels
        self.ctx.newmark_disp_aggregate_grad(T, rho, scaler, components, None, want_G=False, seed_adjoint=True)
        self.ctx.newmark_adjoint_seeded(T)
        self.Lam = self.ctx.newmark_tensor(2)
        g_t, dF = self.residual_T_products()
        return -g_t, -dF

    def von_Mises_stress(self, level=None):
        """Top-surface von Mises stress of one time level as a DG1 field, nvc values per cell (plate_sim.py:446-450)."""
        self._level_state(level)
        return self.ctx.field_output("stress")

    def construct_force_to_pressure_map(self):
        """Consistent mass matrix of the pressure space [CG1]^3 (plate_sim.py:452-468)."""
        from ..rm_shell.rm_shell_pde import force_to_pressure_map
        return force_to_pressure_map(self.mesh)

    def construct_nodal_disp_map(self):
        """Sparse (3 nn x fe_dofs) map history level -> [ux; uy; uz] at the mesh vertices (plate_sim.py:470-480)."""
        from ..rm_shell.rm_shell_pde import nodal_disp_map
        return nodal_disp_map(self.mesh)

    # ------------------------------------------------------------------ outputs on one level
    def assembleStrainEnergy(self, w):
        self.ctx.set_state(np.asarray(w, dtype=np.float64))
        return self.ctx.functional("elastic_energy")

    def strain_energy_gradients(self, w):
        """(dE/dt, dE/dw) of the strain energy at one level."""
        self.ctx.set_state(np.asarray(w, dtype=np.float64))
        return self.ctx.dfunctional("elastic_energy", "thickness"), self.ctx.dfunctional("elastic_energy", "disp_solid")

    def volume(self):
        return self.ctx.functional("volume")

    def dvolume_dt(self):
        return self.ctx.dfunctional("volume", "thickness")

    # ------------------------------------------------------------------ adjoint
    def adjoint_history(self, G):
        """Lambda solving (dR/dy)^T Lambda = G for the whole-history residual R(y) (y = all levels), by the
        backward two-vector recursion
            mu_i = b M lam_{i+1} - mu_{i+1},   A lam_i = G_i + b mu_i + (a M - K/2) lam_{i+1} - b mu_{i+1},
        lam_0 = G_0 + (a M - K/2) lam_1 - b mu_1 (femo_newmark_adjoint).  G, Lambda: (fe_dofs, time_levels)."""
        self._newmark()
        self.ctx.newmark_adjoint(np.ascontiguousarray(np.asarray(G, dtype=np.float64).T))
        self.Lam = self.ctx.newmark_tensor(2)
        return self.ctx.newmark_history(2).T.copy(order="F")

    def residual_T_products(self, Lam_host=None):
        """(sum_i (dR_i/dt)^T lam_i,  [(dR_i/df)^T lam_i]_i) for the displacement history of the last march and the adjoint
        history ``Lam_host`` ((fe_dofs, time_levels); None: the one the last ``adjoint_history`` left on the device)."""
        if Lam_host is not None:
            self.ctx.newmark_set_history(np.ascontiguousarray(np.asarray(Lam_host, dtype=np.float64).T), which=2)
        g, dF = self.ctx.newmark_residual_T(self.time_levels)
        g_sw = np.zeros(self.num_var)
        if self.add_self_weight and self._sw_weights is None:
            g_sw = dF.reshape(self.time_levels, -1, 3)[:, :, 2].sum(axis=0) * self.rho * self._gravity()
        elif self.add_self_weight:
            # R_i = ... - F_sw(t):  (dR_i/dt_e)^T lam = -rho g sum_a lam_z(p_a) int N2_a dS   (BC rows carry no load)
            Lam = self.ctx.newmark_history(2)
            Lam[:, self.bc_dofs] = 0.0
            lz = Lam[1:, :][:, 3 * self.mesh.cell_p2 + 2].sum(axis=0)                 # (nel, npc), summed over the levels 1..
            g_sw = -self.rho * self._gravity() * (self._sw_weights * lz).sum(axis=1)
        return g + g_sw, dF

    # ------------------------------------------------------------------ forward mode (tangent linear model)
    def jacobian_products_fwd(self, dY=None, dthickness=None, dF=None):
        """d_residuals = (dR/dy) dY + (dR/dt) dthickness + (dR/df) dF for the history of the last march
        (state_operation_dynamic.py:228-329), (fe_dofs, time_levels).  dY: (fe_dofs, time_levels); dF: (time_levels, 3 nn)."""
        self._newmark()
        T = self.time_levels
        dFh = None if dF is None else np.asarray(dF, dtype=np.float64).reshape(T, -1, 3).copy()
        extra = None
        if dthickness is not None and self.add_self_weight:
            dth = np.asarray(dthickness, dtype=np.float64).ravel()
            if self._sw_weights is None:                   # nodal thickness: the self weight rides on the pressure, f_z += rho g dt
                if dFh is None:
                    dFh = np.zeros((T, self.nn, 3))
                dFh[:, :, 2] += (self.rho * self._gravity() * dth)[None, :]
            else:                                          # element-wise thickness: R_i = ... - F_sw(t)
                extra = np.zeros(self.fe_dofs)
                np.add.at(extra, 3 * self.mesh.cell_p2.ravel() + 2, (self._sw_weights * (self.rho * self._gravity() * dth)[:, None]).ravel())
                extra[self.bc_dofs] = 0.0
        out = self.ctx.newmark_jvp(T, None if dY is None else np.ascontiguousarray(np.asarray(dY, dtype=np.float64).T),
                                   dthickness, None if dFh is None else dFh.reshape(T, -1))
        if extra is not None:
            out[1:] -= extra[None, :]
        return out.T.copy(order="F")

    def tangent_history(self, dR):
        """dY solving (dR/dy) dY = dR level by level -- the direct method of state_operation_dynamic.py:534-605.
        dR, dY: (fe_dofs, time_levels)."""
        self._newmark()
        return self.ctx.newmark_tangent(np.ascontiguousarray(np.asarray(dR, dtype=np.float64).T)).T.copy(order="F")
