"""``RMShellModel``: the model facade example scripts call.

Constructor and ``evaluate`` follow femo_alpha/rm_shell/rm_shell_model.py:31-81,364-490; the
``mesh`` argument is a ``femo_alpha_amd.mesh.ShellMesh`` (nodes + connectivity, the data
``reconstructFEAMesh`` takes) instead of a dolfinx mesh.  Outputs, as in the reference:
``disp_solid`` (state), ``compliance``, ``mass``, ``elastic_energy``, ``pnorm_stress``, the DG1 field
``stress``, ``disp_extracted`` and ``aggregated_stress``.
"""
from __future__ import annotations

import numpy as np

from .. import csdl
from ..csdl_alpha_opt.fea_model import FEAModel
from ..fea.fea_hip import FEA, DirichletBC, Function
from ..mesh import ShellMesh
from .rm_shell_pde import FacetSet, RMShellPDE


def solve_linear(A, b, ctx):
    """pressure = A^-1 force as a differentiable node: ``csdl.solve_linear`` when csdl_alpha is installed (what the
    reference calls, rm_shell_model.py:420); otherwise an explicit operation whose solve runs on the device
    (``femo_force_to_pressure``: Jacobi-PCG with the consistent [CG1]^3 mass matrix applied cell by cell -- the matrix ``A`` of
    ``construct_force_to_pressure_map`` is the same operator and is not touched).  ``ctx``: the shell context whose device runs
    that solve (required: there is no host fallback)."""
    if csdl.HAVE_CSDL_ALPHA:
        return csdl.solve_linear(A.toarray(), b)
    if ctx is None:
        raise ValueError("solve_linear: without csdl_alpha the force -> pressure solve runs on the device and needs the shell context")

    class _Solve(csdl.CustomExplicitOperation):
        def evaluate(self, rhs):
            self.declare_input("b", rhs)
            x = self.create_output("x", rhs.shape)
            self.declare_derivative_parameters("x", "*", dependent=True)
            self._finish_evaluate()
            return x

        def compute(self, input_vals, output_vals):
            output_vals["x"] = ctx.force_to_pressure(np.asarray(input_vals["b"], dtype=np.float64))

        def vjp(self, bar):                      # A is symmetric: bar_b = A^-T bar_x
            return ctx.force_to_pressure(bar)

    return _Solve().evaluate(b)


def createCustomMeasure(mesh: ShellMesh, dim, SubdomainFunc, measure: str, tag: int):
    """Tagged facet measure (femo_alpha/fea/utils_dolfinx.py:555-565): 'ds' = boundary facets whose
    vertices all satisfy the marker, 'dS' = interior facets, integrated from both sides."""
    if dim != 1:
        raise ValueError("shell facets have dimension 1")
    if measure == "ds":
        ed = mesh.locate_facets(SubdomainFunc, boundary_only=True)
        pairs = np.stack([mesh.edge_cells[ed, 0], mesh.edge_local[ed, 0]], axis=1)
    else:
        ed = mesh.locate_facets(SubdomainFunc, boundary_only=False)
        ed = ed[mesh.edge_cells[ed, 1] >= 0]
        if mesh.is_manifold:
            pairs = np.vstack([np.stack([mesh.edge_cells[ed, s], mesh.edge_local[ed, s]], axis=1) for s in (0, 1)])
        else:
            pairs = mesh.facet_incidence(ed)           # branching edges: every incident cell
    sets = {tag: FacetSet(pairs)}
    return lambda t: sets.get(t, FacetSet(np.zeros((0, 2), np.int32)))


class RMShellModel:
    def __init__(self, mesh: ShellMesh, shell_bc_func: callable = None, element_wise_material=False, rho=100,
                 PENALTY_BC=True, additional_outputs=None, mesh_tags=None, record=True, elementwise_pressure=False,
                 device=0, renumber=False, nquad=None, laminate=False, ply_failure=None, layup=None, max_disp=None,
                 ply_strength=False, hashin=False):
        # caller order <-> solver order.  dolfinx reorders every mesh it is given and the reference carries the maps
        # (rm_shell_model.py:116, 396-438, 505-527); with renumber=True this build does the same with a Morton order of
        # the cells (ShellMesh.renumbered): inputs are gathered into solver order, nodal displacements come back in
        # caller order, the state ``disp_solid`` lives in solver order as it does in the reference.
        self.caller_mesh = mesh
        if renumber:
            mesh, self.vertex_of_new, self.cell_of_new = mesh.renumbered()
        else:
            self.vertex_of_new, self.cell_of_new = np.arange(mesh.nn), np.arange(mesh.nel)
        self.new_of_vertex = np.empty(mesh.nn, dtype=np.int64)
        self.new_of_vertex[self.vertex_of_new] = np.arange(mesh.nn)
        self.new_of_cell = np.empty(mesh.nel, dtype=np.int64)
        self.new_of_cell[self.cell_of_new] = np.arange(mesh.nel)
        if mesh_tags is not None:
            for inds in mesh_tags.values():
                inds = np.asarray(inds, dtype=np.int64)
                if inds.size and (inds.min() < 0 or inds.max() >= mesh.nel):
                    raise ValueError("mesh_tags: cell index out of range")
            mesh_tags = {tag: self.new_of_cell[np.asarray(inds, dtype=np.int64)] for tag, inds in mesh_tags.items()}
        self.mesh = mesh
        self.mesh_tags = mesh_tags
        self.additional_outputs = additional_outputs
        self.shell_bc_func = shell_bc_func
        self.element_wise_material = element_wise_material
        self.record = record
        self.m, self.rho = 1e-6, rho
        self.PENALTY_BC = PENALTY_BC
        self.nel, self.nn = mesh.nel, mesh.nn
        self.elementwise_pressure = elementwise_pressure
        self.device = device
        # laminate=True: the composite law with a DG0 "laminate" input of (nel, 32) values per cell in caller order
        # ([A, B, D, A_s, c_drill], femo_alpha_amd.laminate.pack), an argument of disp_solid and elastic_energy
        self.laminate = bool(laminate)
        # ply_failure=npt (with laminate=True): a DG0 "ply_table" input of (nel, npt, 16) values in caller cell order
        # (femo_alpha_amd.laminate.ply_table) and the output "ply_failure", the KS aggregate of the ply failure index
        self.ply_failure = None if ply_failure is None else int(ply_failure)
        if self.ply_failure is not None and not self.laminate:
            raise ValueError("ply_failure needs laminate=True")
        # layup=dict(plies, t, theta[, surfaces, c_drill, density]) (with laminate=True; ShellContext.set_layup): the design variables of the
        # laminate are the inputs "ply_thickness" and "ply_angle", (nel, nply) in caller cell order, and the laminate and the ply table
        # are built from them on the device.  t and theta give the initial layup ((nply,) or (nel, nply) in caller cell order); with
        # recovery points (surfaces, default bot / top of every ply) the output "ply_failure" exists.  They take the place of the
        # laminate= and ply_table= arguments of evaluate and of ply_failure=npt here.  The outputs "layup_volume" and, with the (nply,)
        # ply densities density=[...], "layup_mass" are functions of "ply_thickness" and "uhat" alone.  With the (nply, 2) transverse
        # shear strengths shear_strength=[[S13, S23], ...] the output "ply_shear_failure" exists, with the arguments of "ply_failure".
        # reference="mid" | "bot" | "top" | r and offset (a length, or (nel,) in caller cell order) choose the reference surface the mesh
        # stands for (ShellContext.set_layup_reference); the default is the mid-surface.
        self.layup = None
        if layup is not None:
            if not self.laminate or self.ply_failure is not None:
                raise ValueError("layup needs laminate=True, and its surfaces take the place of ply_failure=npt")
            t, theta = (np.asarray(layup[k], dtype=np.float64) for k in ("t", "theta"))
            nply = t.shape[-1] if t.ndim else 1
            to_solver = lambda a: np.broadcast_to(a.reshape(-1, nply), (mesh.nel, nply))[self.cell_of_new]
            self.layup = dict(layup, t=to_solver(t), theta=to_solver(theta))
            if layup.get("offset") is not None and np.ndim(layup["offset"]):
                # the per-cell offsets of the reference surface arrive in caller cell order, as t and theta do
                self.layup["offset"] = np.broadcast_to(np.asarray(layup["offset"], dtype=np.float64).ravel(), (mesh.nel,))[self.cell_of_new]
            self.nply = nply
        # max_disp=dict(...) or a list of up to four: one max-displacement output per dict (RMShellPDE.max_disp) with the keys rho,
        # scaler, direction, nodes, name (default "max_disp", "max_disp1", ...) and tag (a key of mesh_tags; none: the whole mesh).  The
        # slot is the position in the list.
        # ply_strength=True (opt-in; with ply_failure=npt or a layup): the output "ply_strength_index", the KS aggregate of the
        # load-proportional strength index r = 1 / (strength ratio) on the same ply table, with the arguments "ply_failure" has
        self.ply_strength = bool(ply_strength)
        if self.ply_strength and self.ply_failure is None and layup is None:
            raise ValueError("ply_strength needs a ply table: ply_failure=npt or a layup")
        if self.ply_strength and layup is not None and not len(tuple(layup.get("surfaces", ("bot", "top")))):
            raise ValueError("ply_strength needs a ply table: this layup has no recovery points (surfaces)")
        # hashin (opt-in; with laminate=True and a ply table): the outputs "ply_hashin_fibre" and "ply_hashin_matrix", the KS
        # aggregates of the Hashin fibre and matrix failure indices, beside "ply_failure" and with its arguments.  The strengths
        # [Xt, Xc, Yt, Yc, SL, ST] are the same in every cell: with a layup hashin=True reads them from the layup's "hashin" key or
        # from its ply dicts (Xt, Xc, Yt, Yc, S, optionally ST), and hashin=(nply, 6) | (6,) | ply dicts gives them here; with
        # ply_failure=npt hashin=(npt, 6) | (6,).  Strengths that vary over the cells go to ShellContext.set_ply_hashin_table.
        self.hashin = None if hashin is None or hashin is False else hashin
        if self.hashin is not None:
            if not self.laminate:
                raise ValueError("hashin needs laminate=True")
            if self.ply_failure is None and layup is None:
                raise ValueError("hashin needs a ply table: ply_failure=npt or a layup")
            if layup is not None and not len(tuple(layup.get("surfaces", ("bot", "top")))):
                raise ValueError("hashin needs a ply table: this layup has no recovery points (surfaces)")
            if self.hashin is not True and np.ndim(self.hashin) > 2:
                raise ValueError("hashin: strengths per ply or per recovery point, the same in every cell")
            if self.hashin is True and layup is None:
                raise ValueError("hashin=True reads the strengths of a layup; with ply_failure=npt give hashin=[Xt, Xc, Yt, Yc, SL, ST]")
        self.max_disp = None
        if max_disp is not None:
            specs = [dict(max_disp)] if isinstance(max_disp, dict) else [dict(d) for d in max_disp]
            if not 1 <= len(specs) <= 4:
                raise ValueError("max_disp: one to four outputs")
            known = {"rho", "scaler", "direction", "nodes", "name", "tag"}
            names = set()
            for i, d in enumerate(specs):
                if set(d) - known:
                    raise ValueError(f"max_disp: unknown keys {sorted(set(d) - known)}")
                d.setdefault("name", "max_disp" + (str(i) if i else ""))
                if d.get("tag") is not None and (mesh_tags is None or d["tag"] not in mesh_tags):
                    raise ValueError(f"max_disp: tag '{d['tag']}' is not a key of mesh_tags")
                if d["name"] in names:
                    raise ValueError(f"max_disp: the name '{d['name']}' is used twice")
                names.add(d["name"])
            self.max_disp = specs
        # n x n Gauss points per quadrilateral for the static forms (2..5).  The reference leaves the degree to UFL's
        # estimate, which on quadrilaterals comes out near 47 (scripts/ufl_degree_estimate.py): exact integration.  Default:
        # what the mesh asks for -- 4 on affine cells (exact there), 5 as soon as one cell is warped (within 1e-9 of the
        # limit at BASELINE config 3; ShellMesh.recommended_nquad).
        # On triangles nquad is the degree of the symmetric rule: 6 (exact for cell-wise polynomial data), and the context raises it to
        # UFL's 9 by itself when a nodal Poisson ratio that varies over the cells arrives -- unless the caller names the rule here.
        self._nquad_arg = None if nquad is None else int(nquad)
        self.association_table = None
        if shell_bc_func is None:
            raise ValueError("Please provide the shell bc location function.\n"
                             " Example:\n def ClampedBoundary(x):\n    return np.less(x[1], 0.0)")
        self.set_up_bcs(shell_bc_func, PENALTY_BC)
        self.set_up_fea()

    @property
    def nquad(self):
        """The rule in use (ShellContext.nquad)."""
        return self.shell_pde.ctx.nquad

    def set_up_subdomains(self, mesh_tags):
        """mesh_tags: {tag: [cell indices]} without duplicates (rm_shell_model.py:101-133).  Builds
        ``association_table`` {tag: sub-domain index} and hands the per-cell index array to the backend."""
        vals = -np.ones(self.mesh.nel, dtype=np.int32)
        for i, inds in enumerate(mesh_tags.values()):
            inds = np.asarray(inds, dtype=np.int64)
            if inds.size and (inds.min() < 0 or inds.max() >= self.mesh.nel):
                raise ValueError("mesh_tags: cell index out of range")
            if np.any(vals[inds] != -1):
                raise ValueError("mesh_tags: a cell may carry one tag only")
            vals[inds] = i
        self.association_table = {key: i for i, key in enumerate(mesh_tags.keys())}
        self.shell_pde.ctx.set_cell_tags(vals, len(mesh_tags))

    def set_up_bcs(self, bc_locs_func, PENALTY_BC):
        if PENALTY_BC:
            self.dss = createCustomMeasure(self.mesh, 1, bc_locs_func, measure="ds", tag=100)(100)
            self.dSS = createCustomMeasure(self.mesh, 1, bc_locs_func, measure="dS", tag=100)(100)
        else:
            self.dss = self.dSS = None

    def set_up_fea(self):
        mesh = self.mesh
        shell_pde = self.shell_pde = RMShellPDE(mesh, element_wise_material=self.element_wise_material,
                                                elementwise_pressure=self.elementwise_pressure, device=self.device,
                                                nquad=self._nquad_arg, laminate=self.laminate, ply_failure=self.ply_failure,
                                                layup=self.layup, hashin=self.hashin)
        fea = FEA(mesh)
        if self.caller_mesh is not mesh:                 # renumbered: FEA.field_tangents answers in caller order
            fea.vertex_of_new, fea.cell_of_new = self.vertex_of_new, self.cell_of_new
        fea.PDE_SOLVER = "Newton"
        fea.REPORT = False
        fea.record = False                    # XDMF recording is out of scope; the flag is accepted and ignored
        fea.linear_problem = True
        h, f = Function(shell_pde.VT), Function(shell_pde.VF)
        E, nu, density = Function(shell_pde.VT), Function(shell_pde.VT), Function(shell_pde.VT)
        uhat = Function(shell_pde.VU)
        w = Function(shell_pde.W)
        if not self.PENALTY_BC:
            dofs = mesh.locate_dofs_geometrical(self.shell_bc_func)
            shell_pde.ctx.set_strong_dofs(dofs)
            fea.bc = [DirichletBC(dofs)]
        g = Function(shell_pde.W)
        residual_form = shell_pde.pdeRes(h=h, w=w, uhat=uhat, f=f, E=E, nu=nu, penalty=self.PENALTY_BC,
                                         dss=self.dss, dSS=self.dSS, g=g)
        compliance_form = shell_pde.compliance(w, uhat, h, f)
        mass_form = shell_pde.mass(uhat, h, density)
        elastic_energy_form = shell_pde.elastic_energy(w, uhat, h, E)
        pnorm_stress_form = shell_pde.pnorm_stress(w, uhat, h, E, nu, None, m=self.m, rho=self.rho, alpha=None,
                                                   regularization=False)
        stress_form = shell_pde.von_Mises_stress(w, uhat, h, E, nu, surface="Top")
        fea.add_input("thickness", h, init_val=0.001)
        fea.add_input("F_solid", f, init_val=1.0)
        fea.add_input("E", E, init_val=1.0)
        fea.add_input("nu", nu, init_val=1.0)
        fea.add_input("density", density, init_val=1.0)
        fea.add_input("uhat", uhat, init_val=0.0)
        lam_args = []
        if self.layup is not None:
            ply_t = Function(shell_pde.VY).bind("ply_thickness")
            ply_a = Function(shell_pde.VY).bind("ply_angle")
            fea.add_input("ply_thickness", ply_t, init_val=shell_pde.ply_thickness_init)
            fea.add_input("ply_angle", ply_a, init_val=shell_pde.ply_angle_init)
            lam_args = ["ply_thickness", "ply_angle"]
        elif self.laminate:
            lam = Function(shell_pde.VL).bind("laminate")
            fea.add_input("laminate", lam, init_val=shell_pde.laminate_init)
            lam_args = ["laminate"]
        fea.add_state(name="disp_solid", function=w, residual_form=residual_form,
                      arguments=["thickness", "F_solid", "E", "nu", "uhat"] + lam_args)
        fea.add_output(name="compliance", form=compliance_form, arguments=["disp_solid", "F_solid", "thickness", "uhat"])
        fea.add_output(name="mass", form=mass_form, arguments=["thickness", "density", "uhat"])
        fea.add_output(name="elastic_energy", form=elastic_energy_form, arguments=["thickness", "disp_solid", "E", "uhat"] + lam_args)
        fea.add_output(name="pnorm_stress", form=pnorm_stress_form, arguments=["thickness", "disp_solid", "E", "nu", "uhat"])
        if self.layup is not None and shell_pde.ply_npt:
            fea.add_output(name="ply_failure", form=shell_pde.ply_failure(w, uhat, None, rho=self.rho), arguments=["disp_solid"] + lam_args)
        if self.layup is not None and shell_pde.ply_npt and self.ply_strength:
            fea.add_output(name="ply_strength_index", form=shell_pde.ply_strength_index(w, uhat, None, rho=self.rho),
                           arguments=["disp_solid"] + lam_args)
        if self.layup is not None and shell_pde.ply_npt and self.hashin is not None:
            for mode in ("fibre", "matrix"):
                fea.add_output(name="ply_hashin_" + mode, form=shell_pde.ply_hashin(w, uhat, None, mode, rho=self.rho),
                               arguments=["disp_solid"] + lam_args)
        if self.layup is not None and shell_pde.layup_shear:
            # shear_strength=[...] in the layup: the interlaminar shear aggregate, with the arguments ply_failure has on this route
            fea.add_output(name="ply_shear_failure", form=shell_pde.ply_shear_failure(w, uhat, None, rho=self.rho),
                           arguments=["disp_solid"] + lam_args)
        if self.layup is not None:
            if shell_pde.layup_density:
                fea.add_output(name="layup_mass", form=shell_pde.layup_mass(uhat, ply_t), arguments=["ply_thickness", "uhat"])
            fea.add_output(name="layup_volume", form=shell_pde.layup_volume(uhat, ply_t), arguments=["ply_thickness", "uhat"])
        if self.ply_failure is not None:
            ply = Function(shell_pde.VP).bind("ply_table")
            fea.add_input("ply_table", ply, init_val=shell_pde.ply_table_init)
            fea.add_output(name="ply_failure", form=shell_pde.ply_failure(w, uhat, ply, rho=self.rho), arguments=["disp_solid", "ply_table"])
            if self.ply_strength:
                fea.add_output(name="ply_strength_index", form=shell_pde.ply_strength_index(w, uhat, ply, rho=self.rho),
                               arguments=["disp_solid", "ply_table"])
            if self.hashin is not None:
                for mode in ("fibre", "matrix"):
                    fea.add_output(name="ply_hashin_" + mode, form=shell_pde.ply_hashin(w, uhat, ply, mode, rho=self.rho),
                                   arguments=["disp_solid", "ply_table"])
        if self.mesh_tags is not None:
            self.set_up_subdomains(self.mesh_tags)
            for tag, i in self.association_table.items():
                # a stress aggregate per sub-domain, named after the caller's tag (rm_shell_model.py:242-253)
                form_i = shell_pde.pnorm_stress(w, uhat, h, E, nu, i, m=self.m, rho=self.rho, alpha=None, regularization=False)
                fea.add_output(name="pnorm_stress_" + str(tag), form=form_i,
                               arguments=["thickness", "disp_solid", "E", "nu", "uhat"])
        for i, d in enumerate(self.max_disp or ()):
            if d["name"] in fea.outputs_dict or d["name"] in fea.inputs_dict or d["name"] in fea.states_dict:
                raise ValueError(f"max_disp: the name '{d['name']}' is taken")
            dx = None if d.get("tag") is None else self.association_table[d["tag"]]
            form_i = shell_pde.max_disp(w, dx, slot=i, rho=d.get("rho", 100.0), scaler=d.get("scaler", 1.0),
                                        direction=d.get("direction"), nodes=d.get("nodes", "vertices"))
            fea.add_output(name=d["name"], form=form_i, arguments=["disp_solid"])
        fea.add_field_output(name="stress", form=stress_form, arguments=["thickness", "disp_solid", "E", "nu", "uhat"],
                             function_space=("DG", 1), record=False, vtk=True)
        if self.layup is not None and shell_pde.ply_npt:
            self.ply_failure_field_form = shell_pde.ply_failure_field(w, uhat, None)
        if self.layup is not None and shell_pde.layup_shear:
            self.ply_shear_failure_field_form = shell_pde.ply_shear_failure_field(w, uhat, None)
        if self.ply_failure is not None:
            # (nel, npt) flattened, differentiated through FEA.field_tangents (forward) and FEA.field_gradients (reverse: local failure
            # constraints in groups of four adjoint solves); registering it as a field output of the CSDL model is a separate step
            self.ply_failure_field_form = shell_pde.ply_failure_field(w, uhat, ply)
        if self.ply_strength and (self.ply_failure is not None or shell_pde.ply_npt):
            self.ply_strength_index_field_form = shell_pde.ply_strength_index_field(w, uhat, None)
        if self.hashin is not None:
            self.ply_hashin_fibre_field_form = shell_pde.ply_hashin_field(w, uhat, None, "fibre")
            self.ply_hashin_matrix_field_form = shell_pde.ply_hashin_field(w, uhat, None, "matrix")
        self.fea = fea

    def evaluate(self, force_vector, thickness, E, nu, density, node_disp=None, debug_mode=False, is_pressure=True, laminate=None,
                 ply_table=None, ply_thickness=None, ply_angle=None):
        """laminate: (nel, 32) per cell in caller order -- required with laminate=True, refused otherwise.  thickness, E, nu and density
        stay inputs in laminate mode (mass, regularisation, stress outputs).  ply_table: (nel, npt, 16) per cell in caller order --
        required with ply_failure=npt, refused otherwise.  With layup=...: ply_thickness and ply_angle, (nel, nply) in caller cell
        order, are required, and laminate / ply_table are refused."""
        if (self.layup is not None) != (ply_thickness is not None and ply_angle is not None) or \
                (self.layup is None and (ply_thickness is not None or ply_angle is not None)):
            raise ValueError("ply_thickness and ply_angle are required with layup=... and refused without it")
        if self.layup is not None and (laminate is not None or ply_table is not None):
            raise ValueError("with layup=... the laminate and the ply table are built from ply_thickness and ply_angle")
        if self.layup is None and self.laminate != (laminate is not None):
            raise ValueError("a laminate is required with laminate=True and refused without it")
        if (self.ply_failure is not None) != (ply_table is not None):
            raise ValueError("a ply_table is required with ply_failure=npt and refused without it")
        shell_inputs = csdl.VariableGroup()
        mesh = self.mesh
        # caller order == solver order here; the gathers are kept so that a renumbered mesh object
        # can plug in its permutations exactly where the reference applies them (:398-438)
        mat_idx = self.cell_of_new if self.element_wise_material else self.vertex_of_new
        shell_inputs.thickness = thickness[mat_idx]
        shell_inputs.E = E[mat_idx]
        shell_inputs.nu = nu[mat_idx]
        shell_inputs.density = density[mat_idx]
        prs_idx = self.cell_of_new if self.elementwise_pressure else self.vertex_of_new
        reshaped_force = csdl.reshape(force_vector[prs_idx], (-1,))
        if is_pressure:
            shell_inputs.F_solid = reshaped_force
        else:
            # nodal forces -> nodal pressures through the consistent mass matrix (rm_shell_model.py:414-421)
            # the matrix itself is only needed by csdl_alpha's solve_linear; the stand-in solves on the device
            if self.elementwise_pressure:          # as construct_force_to_pressure_map says, with or without csdl_alpha
                raise NotImplementedError("force -> pressure conversion is defined for nodal pressures")
            A = self.shell_pde.construct_force_to_pressure_map() if csdl.HAVE_CSDL_ALPHA else None
            shell_inputs.F_solid = solve_linear(A, reshaped_force, ctx=self.shell_pde.ctx)
        shell_inputs.F_solid.add_name("F_solid")
        if node_disp is None:
            node_disp = csdl.Variable(value=0.0, shape=(mesh.nn, 3), name="node_disp")
        reshaped_node_disp = node_disp[self.vertex_of_new].reshape((-1,))
        reshaped_node_disp.add_name("uhat")
        shell_inputs.uhat = reshaped_node_disp
        for n in ("thickness", "E", "nu", "density"):
            getattr(shell_inputs, n).add_name(n)
        if self.layup is not None:
            shell_inputs.ply_thickness = ply_thickness[self.cell_of_new].reshape((-1,))      # caller cell order -> solver order
            shell_inputs.ply_thickness.add_name("ply_thickness")
            shell_inputs.ply_angle = ply_angle[self.cell_of_new].reshape((-1,))
            shell_inputs.ply_angle.add_name("ply_angle")
        elif self.laminate:
            shell_inputs.laminate = laminate[self.cell_of_new].reshape((-1,))      # caller cell order -> solver order
            shell_inputs.laminate.add_name("laminate")
        if self.ply_failure is not None:
            shell_inputs.ply_table = ply_table[self.cell_of_new].reshape((-1,))    # caller cell order -> solver order
            shell_inputs.ply_table.add_name("ply_table")

        solid_model = FEAModel(fea=[self.fea], fea_name="rm_shell")
        shell_outputs = solid_model.evaluate(shell_inputs, debug_mode=debug_mode)

        disp_extracted = DisplacementExtractionModel(shell_pde=self.shell_pde).evaluate(shell_outputs.disp_solid)
        disp_extracted = disp_extracted[self.new_of_vertex]              # solver order -> caller order
        disp_extracted.add_name("disp_extracted")
        shell_outputs.disp_extracted = disp_extracted
        aggregated_stress = AggregatedStressModel(m=self.m, rho=self.rho).evaluate(shell_outputs.pnorm_stress)
        aggregated_stress.add_name("aggregated_stress")
        shell_outputs.aggregated_stress = aggregated_stress
        return shell_outputs


class AggregatedStressModel:
    """aggregated_stress = pnorm^(1/rho) / m (rm_shell_model.py:493-503)."""

    def __init__(self, m: float, rho: int):
        self.m, self.rho = m, rho

    def evaluate(self, pnorm_stress):
        return 1 / self.m * pnorm_stress ** (1 / self.rho)


class DisplacementExtractionModel:
    """(nn, 3) vertex displacements in caller node order (rm_shell_model.py:505-527)."""

    def __init__(self, shell_pde: RMShellPDE):
        self.shell_pde = shell_pde

    def evaluate(self, disp_vec):
        nn = self.shell_pde.mesh.nn
        return disp_vec[np.arange(3 * nn)].reshape((nn, 3))


class ForceReshapingModel:
    def __init__(self, shell_pde: RMShellPDE):
        self.shell_pde = shell_pde

    def evaluate(self, nodal_force_mat):
        return csdl.reshape(nodal_force_mat[np.arange(self.shell_pde.mesh.nn)], (-1,))
