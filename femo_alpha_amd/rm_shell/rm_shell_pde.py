"""``RMShellPDE``: the shell's spaces, residual and output forms, resident on one MI355X.

Interface of femo_alpha/rm_shell/rm_shell_pde.py:21-110,173-293.  Where the reference builds UFL
expressions from dolfinx Functions, this class binds ``Function`` handles to the roles they play
in the residual ('thickness', 'F_solid', 'E', 'nu', 'uhat', state) and returns named forms that
libfemo_hip evaluates with hand-written kernels (femo_alpha_amd/csrc/shell_device.h).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from ..backend import PENALTY_BETA, ShellContext
from ..fea.fea_hip import FieldForm, Form, Function, FunctionSpace, ResidualForm


class FacetSet:
    """What a tagged ``ds(100)`` / ``dS(100)`` measure integrates over: (cell, local edge) pairs."""

    def __init__(self, pairs):
        self.pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)


class RMShellPDE:
    def __init__(self, mesh, element_wise_material=False, elementwise_pressure=False, nquad=None, device=0, solver="direct",
                 element_type=None, laminate=False, ply_failure=None, layup=None, hashin=None):
        # element_type: 'CG2CG1' (what the reference's RMShellPDE hard-codes, rm_shell_pde.py:27) or 'CG1CG1' (the other quadrilateral /
        # triangle choice of ShellElement.setUpFunctionSpace, linear_shell_model.py:74-79); None: the element the mesh object carries
        if element_type is not None and element_type != mesh.element:
            from ..mesh import ShellMesh
            mesh = ShellMesh(mesh.nodes, mesh.cells, element_type)
        self.mesh = mesh
        self.element_wise_material = element_wise_material
        self.elementwise_pressure = elementwise_pressure
        self.ctx = ShellContext(mesh, element_wise_material, elementwise_pressure, nquad=nquad, device=device)
        # the reference always solves with a sparse direct LU (MUMPS through PETSc, fea/utils_dolfinx.py:466,514-531):
        # the drop-in surface does the same unless the caller opts out ('jacobi': matrix-free Jacobi-PCG, thick plates only)
        if solver == "direct":
            self.ctx.use_direct_solver()
        elif solver != "jacobi":
            raise ValueError("solver must be 'direct' or 'jacobi'")
        self.W = FunctionSpace(self.ctx, "W")          # [CG2]^3 x [CG1]^3, linear_shell_model.py:60-65
        self.VT = FunctionSpace(self.ctx, "VT")        # rm_shell_pde.py:37-40
        self.VF = FunctionSpace(self.ctx, "VF")        # :41-44
        self.VU = FunctionSpace(self.ctx, "VU")        # :45
        # laminate=True: the composite law (MaterialModelComposite, linear_shell_model.py:159-190) with per-cell CLT data, a DG0 space
        # of 32 values per cell [A, B, D, A_s, c_drill] (femo_alpha_amd.laminate.pack).  The context enters laminate mode at once with a
        # one-ply placeholder (1 mm of a unit-modulus isotropic ply) that the model's "laminate" input replaces.
        self.laminate = bool(laminate)
        self.VL = None
        # layup=dict(plies, t, theta[, surfaces, c_drill, density, shear_strength, reference, offset]) (laminate mode; ShellContext.set_layup, solver cell order): the
        # laminate and the ply table are built on the device from ply thicknesses and angles, two DG0 spaces of nply values per cell; the
        # recovery points, hence "ply_failure", follow from the layup's surfaces, "layup_mass" from its (nply,) ply densities, and
        # "ply_shear_failure" from its (nply, 2) transverse shear strengths [S13, S23]
        # hashin: the strengths [Xt, Xc, Yt, Yc, SL, ST] of the Hashin outputs "ply_hashin_fibre" / "ply_hashin_matrix".  With a layup:
        # per ply, (nply, 6), (6,), ply dicts, or True for the dicts of the layup's plies (the layup's own "hashin" key does the
        # same); with ply_failure=npt: (npt, 6) or (6,) for every cell, or (nel, npt, 6) in solver cell order
        self.hashin = False
        given = hashin is not None and hashin is not False
        if given and not self.laminate:
            raise ValueError("hashin needs laminate=True")
        self.layup = layup
        self.VY = None
        if layup is not None:
            if not self.laminate or ply_failure is not None:
                raise ValueError("layup needs laminate=True, and its surfaces take the place of ply_failure=npt")
            t = np.asarray(layup["t"], dtype=np.float64)
            nply = t.shape[-1] if t.ndim else 1
            surfaces = tuple(layup.get("surfaces", ("bot", "top")))
            strengths = layup.get("hashin")
            if given and not (hashin is True and strengths is not None):
                strengths = hashin
            if strengths is not None and not len(surfaces):
                raise ValueError("hashin needs a ply table: this layup has no recovery points (surfaces)")
            self.ctx.set_layup(layup["plies"], t, layup["theta"], surfaces, layup.get("c_drill"), density=layup.get("density"),
                               shear_strength=layup.get("shear_strength"), reference=layup.get("reference"),
                               offset=layup.get("offset"), hashin=strengths)
            self.hashin = strengths is not None
            self.layup_density = layup.get("density") is not None
            self.layup_shear = layup.get("shear_strength") is not None
            self.VY = FunctionSpace(self.ctx, "VY", width=nply)
            self.ply_thickness_init = self.ctx.get_field("ply_thickness")
            self.ply_angle_init = self.ctx.get_field("ply_angle")
            self.ply_npt = nply * len(surfaces) or None
            self.VP = None
            return
        if self.laminate:
            from ..laminate import isotropic
            self.VL = FunctionSpace(self.ctx, "VL")
            self.laminate_init = isotropic(np.full(mesh.nel, 1e-3), 1.0, 0.3).ravel()
            self.ctx.set_laminate(self.laminate_init)
        # ply_failure=npt (laminate mode): the ply failure aggregate over npt recovery points per cell, a DG0 space of 16 npt values per
        # cell (femo_alpha_amd.laminate.ply_table).  The placeholder table is all zeros (FI = 0) until the model's input replaces it.
        self.ply_npt = None if ply_failure is None else int(ply_failure)
        self.VP = None
        if self.ply_npt is not None:
            if not self.laminate:
                raise ValueError("ply_failure needs laminate=True")
            self.VP = FunctionSpace(self.ctx, "VP", width=16 * self.ply_npt)
            self.ply_table_init = np.zeros(self.VP.dim)
            self.ctx.set_ply_table(self.ply_table_init, self.ply_npt)
        if given:
            if self.ply_npt is None or hashin is True:
                raise ValueError("hashin needs a ply table and strengths: a layup, or ply_failure=npt with hashin=[Xt, Xc, Yt, Yc, SL, ST]")
            self.ctx.set_ply_hashin_table(hashin, npt=None if np.ndim(hashin) < 3 else self.ply_npt)
            self.hashin = True

    # ------------------------------------------------------------------ residual
    def pdeRes(self, h, w, uhat, f, E, nu, penalty=False, dss=None, dSS=None, g=None):
        """Residual of the elastic energy + penalty - load (rm_shell_pde.py:50-58,
        linear_shell_model.py:308-333).  ``g``: the prescribed state of the penalty term (a Function on W; the reference's
        model passes zeros, rm_shell_model.py:183-185); values on strongly imposed DOFs are not used (those are homogeneous,
        as in the reference, rm_shell_model.py:168-180)."""
        h.bind("thickness"); w.bind("state"); uhat.bind("uhat"); f.bind("F_solid"); E.bind("E"); nu.bind("nu")
        if g is not None:
            if not penalty and np.any(g.get()):
                raise NotImplementedError("prescribed values need the penalty treatment (PENALTY_BC=True)")
            g0 = g.get()
            g.bind("dirichlet")
            g.set(g0)
        if penalty:
            pairs = [s.pairs for s in (dss, dSS) if s is not None]
            self.ctx.set_penalty_facets(np.vstack(pairs) if pairs else np.zeros((0, 2), np.int32), PENALTY_BETA)
        return ResidualForm(self.ctx)

    # ------------------------------------------------------------------ outputs
    def compliance(self, u_mid, uhat, h, f):
        """int u.u J dx + regularisation(h) (rm_shell_pde.py:85-89)."""
        return Form(self.ctx, "compliance")

    def regularization(self, h, type=None):
        """Thickness regularisation added to the compliance (rm_shell_pde.py:64-83): 'H1' for nodal thickness,
        'L2' for element-wise thickness -- the two the reference's compliance uses; None means no regularisation."""
        if type is None:
            return 0.0
        expected = "L2" if self.element_wise_material else "H1"
        if type != expected:
            raise NotImplementedError(f"regularization type '{type}': the backend provides '{expected}' for this material layout "
                                      "(the one the reference's compliance selects)")
        return Form(self.ctx, "regularization")

    def tip_disp(self, u_mid, uhat, dxx):
        """0.5 int u.u J over the tagged sub-domain ``dxx`` (its index; rm_shell_pde.py:95-96)."""
        return Form(self.ctx, "tip_disp", subdomain=int(dxx))

    def area_subdomain(self, uhat, dxx):
        """int J over the tagged sub-domain ``dxx`` (rm_shell_pde.py:104-105)."""
        return Form(self.ctx, "area", subdomain=int(dxx))

    def sum_stress_subdomain(self, w, uhat, h, E, nu, dxx):
        """The six integrals of the top-surface in-plane stress components over the tagged sub-domain ``dxx``
        (rm_shell_pde.py:130-150): (sum_x, sum_y, sum_z, sum_xy, sum_xz, sum_yz), restated as ShellStressRM.inplaneStress
        writes them (linear_shell_model.py:446-458).  Values only: the reference registers these outputs in commented-out
        code (rm_shell_model.py:255-262), their partials are not implemented."""
        return tuple(Form(self.ctx, "sum_stress_" + c, subdomain=int(dxx)) for c in ("x", "y", "z", "xy", "xz", "yz"))

    def volume(self, uhat, h):
        """int h J dx (rm_shell_pde.py:98-99)."""
        return Form(self.ctx, "volume")

    def mass(self, uhat, h, rho):
        rho.bind("density")
        return Form(self.ctx, "mass")

    def elastic_energy(self, w, uhat, h, E):
        return Form(self.ctx, "elastic_energy")

    def ply_failure(self, w, uhat, ply_table, dx=None, rho=100.0):
        """KS aggregate of the ply failure index over the recovery points of ``ply_table`` (include/femo_hip.h, femo_set_ply_table);
        ``dx``: None for the whole mesh, or the index of a tagged sub-domain."""
        self.ctx.set_ply_failure_params(rho)
        return Form(self.ctx, "ply_failure", subdomain=-1 if dx is None else int(dx))

    def ply_strength_index(self, w, uhat, ply_table, dx=None, rho=100.0):
        """KS aggregate of the load-proportional ply strength index r = 1 / (strength ratio) over the recovery points of the ply
        table (include/femo_hip.h, "ply_strength_index"): the load may grow by 1 / r until the Tsai-Wu index of ``ply_failure``
        reaches one.  ``dx`` as for ``ply_failure``; ``rho`` is the exponent the two aggregates share (femo_set_ply_failure_params)."""
        self.ctx.set_ply_failure_params(rho)
        return Form(self.ctx, "ply_strength_index", subdomain=-1 if dx is None else int(dx))

    def ply_strength_index_field(self, w, uhat, ply_table):
        """The (nel, npt) field of the strength index per cell and recovery point (its largest value over the cell's quadrature
        points) as a field form, in reverse mode only: ``computeMatVecProductBwd(computePartials(form, f), cbar)`` and
        ``FEA.field_gradients``."""
        return FieldForm(self.ctx, "ply_strength_index_field")

    def ply_hashin(self, w, uhat, ply_table, mode, dx=None, rho=100.0):
        """KS aggregate of the Hashin failure index of one ``mode``, "fibre" or "matrix", over the recovery points of the ply table
        (include/femo_hip.h, "ply_hashin_fibre" / "ply_hashin_matrix"; strengths: ``ShellContext.set_ply_hashin_table`` or the
        layup's ``hashin``).  ``dx`` as for ``ply_failure``; ``rho`` is the exponent the ply aggregates share
        (femo_set_ply_failure_params)."""
        if mode not in ("fibre", "matrix"):
            raise ValueError(f"ply_hashin: mode 'fibre' or 'matrix', got {mode!r}")
        self.ctx.set_ply_failure_params(rho)
        return Form(self.ctx, "ply_hashin_" + mode, subdomain=-1 if dx is None else int(dx))

    def ply_hashin_field(self, w, uhat, ply_table, mode):
        """The (nel, npt) field of the Hashin index of one ``mode`` per cell and recovery point (its largest value over the cell's
        quadrature points) as a field form, in reverse mode only: ``computeMatVecProductBwd(computePartials(form, f), cbar)`` and
        ``FEA.field_gradients``."""
        if mode not in ("fibre", "matrix"):
            raise ValueError(f"ply_hashin_field: mode 'fibre' or 'matrix', got {mode!r}")
        return FieldForm(self.ctx, "ply_hashin_" + mode + "_field")

    def ply_shear_failure(self, w, uhat, ply_shear_table, dx=None, rho=100.0):
        """KS aggregate of the interlaminar shear failure index over the recovery points of the shear table (include/femo_hip.h,
        femo_set_ply_shear_table; under a layup with shear strengths the table is the layup's: pass None); ``dx``: None for the whole
        mesh, or the index of a tagged sub-domain."""
        self.ctx.set_ply_shear_params(rho)
        return Form(self.ctx, "ply_shear_failure", subdomain=-1 if dx is None else int(dx))

    def ply_shear_failure_field(self, w, uhat, ply_shear_table):
        """The (nel, npt) field of the interlaminar shear failure index per cell and recovery point as a field form, in reverse mode
        only: ``computeMatVecProductBwd(computePartials(form, f), cbar)`` and ``FEA.field_gradients``."""
        return FieldForm(self.ctx, "ply_shear_failure_field")

    def max_disp(self, w, dx=None, slot=0, rho=100.0, scaler=1.0, direction=None, nodes="vertices"):
        """Smooth maximum over the selected nodes of scaler |u_i| (or, with ``direction`` d, of scaler d.u_i; scaler < 0: a smooth minimum
        of d.u), divided by scaler (include/femo_hip.h, femo_set_disp_aggregate) -- the static examples' ``tip_displacement =
        csdl.maximum(csdl.norm(disp_extracted, axes=(1,)))`` as an output of the library.  ``dx``: None for the whole mesh, or the index
        of a tagged sub-domain; ``slot`` 0..3 names the functional ('max_disp', 'max_disp1', ...) and keeps the parameters of up to four
        such forms apart; ``nodes``: 'vertices' or 'all'."""
        slot = int(slot)
        if not 0 <= slot <= 3:
            raise ValueError("max_disp: slot must be 0..3")
        d = None if direction is None else tuple(float(x) for x in np.asarray(direction, dtype=np.float64).ravel())
        return Form(self.ctx, "max_disp" + (str(slot) if slot else ""), subdomain=-1 if dx is None else int(dx),
                    disp_params=(slot, float(rho), float(scaler), d, str(nodes)))

    def layup_mass(self, uhat, ply_thickness, dx=None):
        """sum_e (sum_k rho_k t_ek) int_e J dx from the ply thicknesses and the ply densities of the layup (include/femo_hip.h,
        femo_set_layup_density); ``dx``: None for the whole mesh, or the index of a tagged sub-domain."""
        return Form(self.ctx, "layup_mass", subdomain=-1 if dx is None else int(dx))

    def layup_volume(self, uhat, ply_thickness, dx=None):
        """sum_e (sum_k t_ek) int_e J dx from the ply thicknesses of the layup; ``dx`` as for ``layup_mass``."""
        return Form(self.ctx, "layup_volume", subdomain=-1 if dx is None else int(dx))

    def ply_failure_field(self, w, uhat, ply_table):
        """The (nel, npt) field of the largest ply failure index per cell and recovery point as a field form: its tangents come
        from ``computeMatVecProductFwd(computePartials(form, f), v)`` and ``FEA.field_tangents``, its reverse products and total
        gradients from ``computeMatVecProductBwd(computePartials(form, f), cbar)`` and ``FEA.field_gradients``, and
        ``assemble(computePartials(form, f), dim=2)`` is its sparse partial Jacobian (state and ply table)."""
        return FieldForm(self.ctx, "ply_failure_field")

    def pnorm_stress(self, w, uhat, h, E, nu, dx=None, m=1e-6, rho=100, alpha=None, regularization=False):
        """1/alpha int (m vm_top)^rho J dx with the degree-4 measure (rm_shell_pde.py:112-128); alpha is the
        reference area, evaluated by the backend on first use."""
        # regularization=True adds 0.5 * 1e3 int h^rho J dx inside the 1/alpha (rm_shell_pde.py:120-122); (m, rho, that coefficient)
        # travel with the form and reach the context when the form is evaluated: two forms with different parameters coexist
        # dx: None for the whole mesh, or the index i of a tagged sub-domain (the reference passes dxx(i))
        sel = -1 if dx is None else int(dx)
        self.ctx.set_stress_alpha(alpha, sel)          # None: the reference area, evaluated by the backend at first use (:123-127)
        return Form(self.ctx, "pnorm_stress", subdomain=sel, stress_params=(float(m), float(rho), 0.5e3 if regularization else 0.0))

    def von_Mises_stress(self, w, uhat, h, E, nu, surface="Top"):
        """von Mises stress at xi2 = h/2 ('Top'), 0 ('Mid') or -h/2 ('Bot') (rm_shell_pde.py:153-165), as a field the
        backend projects onto DG1.  The reference falls through on any other value (it builds a TypeError without raising
        it, :164) and then fails on the undefined name; here the bad argument is refused."""
        names = {"Top": "stress", "Mid": "stress_mid", "Bot": "stress_bot"}
        if surface not in names:
            raise TypeError("Unsupported surface type for stress computation.")
        return FieldForm(self.ctx, names[surface])

    # ------------------------------------------------------------------ maps
    def construct_force_to_pressure_map(self):
        """Consistent mass matrix of the pressure space VF = [CG1]^3, a = int Pv . w dx
        (rm_shell_pde.py:194-209), node-major xyz ordering like ``F_solid``."""
        if self.elementwise_pressure:
            raise NotImplementedError("force -> pressure conversion is defined for nodal pressures")
        return force_to_pressure_map(self.mesh)

    def construct_nodal_disp_map(self):
        """Sparse (3 nn x ndof) map state -> [ux; uy; uz] at the mesh vertices (rm_shell_pde.py:212-221)."""
        return nodal_disp_map(self.mesh)

    def compute_nodal_disp(self, func: Function):
        u = func.get()[: 3 * self.mesh.nn].reshape(-1, 3)
        return u[:, 0].copy(), u[:, 1].copy(), u[:, 2].copy()


def force_to_pressure_map(mesh):
    """Consistent mass matrix of [CG1]^3 on ``mesh``, node-major xyz ordering (rm_shell_pde.py:194-209;
    dynamic_rm_shell/plate_sim.py:452-468).  Host-side set-up map (3x3 Gauss on quads, 3-point rule on triangles; exact
    for the bilinear / linear basis on affine cells)."""
    m = mesh
    X = m.nodes[m.cells]
    if m.is_quad:
        g = np.array([-np.sqrt(0.6), 0.0, np.sqrt(0.6)]); w = np.array([5.0, 8.0, 5.0]) / 9.0
        P = np.array([(a, b) for a in g for b in g]); Wq = np.array([wa * wb for wa in w for wb in w])
        sx, sy = np.array([-1, 1, 1, -1.0]), np.array([-1, -1, 1, 1.0])
        N = 0.25 * (1 + sx[None] * P[:, :1]) * (1 + sy[None] * P[:, 1:])
        dN = np.stack([0.25 * sx[None] * (1 + sy[None] * P[:, 1:]), 0.25 * sy[None] * (1 + sx[None] * P[:, :1])], axis=-1)
    else:
        P = np.array([[1 / 6, 1 / 6], [2 / 3, 1 / 6], [1 / 6, 2 / 3]]); Wq = np.full(3, 1 / 6)
        N = np.stack([1 - P[:, 0] - P[:, 1], P[:, 0], P[:, 1]], axis=1)
        dN = np.broadcast_to(np.array([[-1.0, -1.0], [1.0, 0.0], [0.0, 1.0]]), (3, 3, 2))
    J = np.einsum("ebi,qbk->eqik", X, dN)
    det = np.linalg.norm(np.cross(J[..., 0], J[..., 1]), axis=-1)
    Me = np.einsum("q,eq,qa,qb->eab", Wq, det, N, N)
    nv = m.nvc
    rows = np.repeat(m.cells, nv, axis=1).ravel()
    cols = np.tile(m.cells, (1, nv)).ravel()
    Ms = sp.coo_matrix((Me.ravel(), (rows, cols)), shape=(m.nn, m.nn)).tocsr()
    return sp.kron(Ms, sp.identity(3), format="csr")


def nodal_disp_map(mesh):
    """Sparse (3 nn x ndof) map state -> [ux; uy; uz] at the mesh vertices, the stacking the reference builds from P2 basis
    evaluations (rm_shell_pde.py:212-221; dynamic_rm_shell/plate_sim.py:470-480); vertices are P2 nodes here, so every
    row holds a single 1."""
    nn, ndof = mesh.nn, mesh.ndof
    rows = np.arange(3 * nn)
    cols = (3 * np.arange(nn)[None, :] + np.arange(3)[:, None]).ravel()
    return sp.csr_matrix((np.ones(3 * nn), (rows, cols)), shape=(3 * nn, ndof))
