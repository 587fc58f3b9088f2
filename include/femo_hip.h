/* libfemo_hip.so -- C ABI of the MI355X-native Reissner-Mindlin shell forward + adjoint path.
 *
 * The reference (LSDOlab/femo_alpha) has no FFI seam of its own: its hot path is Python that
 * calls dolfinx / PETSc through pybind11.  This ABI sits *beneath* the
 * Python operator classes the reference exposes, one entry point per dolfinx/PETSc service the
 * reference's operators consume.  Each declaration cites the reference call it replaces
 * (paths relative to /root/reference/femo_alpha).
 *
 * Conventions: every call returns 0 on success, non-zero on failure with a message available
 * from femo_last_error(); all host buffers are owned by the caller, float64 / int32, 1-D;
 * the context owns every device buffer; one context per GPU; not thread-safe; calls are
 * synchronous on return unless stated otherwise.
 *
 * State vector layout (opaque to callers of the reference as well, rm_shell_model.py:505-527):
 *   w = [ u(P2 node 0) xyz ... u(P2 node nP2-1) xyz | theta(vertex 0) xyz ... ]   ndof = 3 nP2 + 3 nn
 */
#ifndef FEMO_HIP_H
#define FEMO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct femo_ctx femo_ctx;

/* Library / device probing ------------------------------------------------------------------ */
int femo_version(void);
int femo_device_count(void);
/* Message of the last failed call on ctx (ctx == NULL: last failed femo_create). */
const char* femo_last_error(const femo_ctx* ctx);

/* Context = mesh + CG2xCG1 numbering on one GPU.
 * Replaces RMShellPDE.__init__ / ShellElement.setUpFunctionSpace (rm_shell/rm_shell_pde.py:25-47,
 * linear_shell_fenicsx/linear_shell_model.py:47-86).
 *   nvc            4 (quads, CCW) or 3 (triangles)
 *   xyz            nn*3 vertex coordinates
 *   cells          nel*nvc vertex ids
 *   cell_p2        nel*npc P2 node ids (npc = 9 quads / 6 triangles: vertices, edge midpoints, centre)
 *   elementwise_material / elementwise_pressure   DG0 instead of CG1 for VT / VF (rm_shell_pde.py:37-44)
 *   nquad          the rule of the static forms (the reference leaves it to UFL's estimate: plain dx, linear_shell_model.py:88-103).
 *                  Quadrilaterals: Gauss points per direction, 2..6.  Triangles: the DEGREE of the fully symmetric rule --
 *                  4 (6 points), 6 (12 points; also what 0 selects), 9 (19 points: UFL's estimate for these forms) or 12 (33 points);
 *                  exact literals of every rule: scripts/derive_triangle_rules.py.  The p-norm stress measure is the reference's
 *                  quadrature_degree 4 whatever nquad says (rm_shell_model.py:200-205): 3 x 3 Gauss / the 6-point rule. */
int femo_create(femo_ctx** out, int device, int32_t nn, int32_t nel, int32_t nvc, int32_t nP2,
                const double* xyz, const int32_t* cells, const int32_t* cell_p2,
                int elementwise_material, int elementwise_pressure, int nquad);
/* The same with nghost extra entries appended to every state-sized vector: DOFs that exist on other
 * element partitions only (replicated separator DOFs of the multi-GPU driver).  femo_ndof then returns
 * mesh DOFs + nghost.  No element kernel touches the extra entries. */
int femo_create_ghost(femo_ctx** out, int device, int32_t nn, int32_t nel, int32_t nvc, int32_t nP2,
                      const double* xyz, const int32_t* cells, const int32_t* cell_p2,
                      int elementwise_material, int elementwise_pressure, int nquad, int32_t nghost);
/* The same with the mixed element chosen explicitly (ShellElement.setUpFunctionSpace, linear_shell_model.py:47-86):
 *   element 0   'CG2CG1' -- or 'CG1CG1' when nP2 == nn -- exactly femo_create_ghost;
 *   element 1   'CG2CR1' (:68-73; triangles only, as in the reference): displacement on the P2 nodes, rotation on the EDGE MIDPOINTS with
 *               the Crouzeix-Raviart functions.  The rotation nodes are the P2 nodes nn .. nP2 - 1 (cell_p2 lists the edge midpoints of a
 *               cell behind its vertices): state vector [u(P2 nodes) xyz | theta(edge midpoints) xyz], femo_ndof = 3 nP2 + 3 (nP2 - nn).
 *               Provided: operator, both Dirichlet treatments, solves, scalar outputs, stress outputs, the adjoint chain for thickness / E /
 *               nu / F_solid / uhat (shape), the transient march with its adjoint, the CSR export, ghost entries (element partitions: the
 *               rotation DOFs of a replicated separator belong to its edge midpoints). */
int femo_create_element(femo_ctx** out, int device, int32_t nn, int32_t nel, int32_t nvc, int32_t nP2,
                        const double* xyz, const int32_t* cells, const int32_t* cell_p2,
                        int elementwise_material, int elementwise_pressure, int nquad, int32_t nghost, int element);
void femo_destroy(femo_ctx* ctx);

int64_t femo_ndof(const femo_ctx* ctx);
/* Length of an input field: "thickness","E","nu","density" (nn or nel), "F_solid" (3*nn or 3*nel), "uhat" (3*nn),
 * "laminate" (32*nel, laminate mode only; -1 otherwise), "ply_table" (16*npt*nel once femo_set_ply_table has set one; -1 otherwise),
 * "ply_shear_table" (6*npt_s*nel once femo_set_ply_shear_table or a layup with shear strengths has set one; -1 otherwise),
 * "ply_thickness", "ply_angle" (nel*nply while a layup is active, femo_set_layup; -1 otherwise). */
int64_t femo_field_size(const femo_ctx* ctx, const char* name);

/* Dirichlet data.
 * Penalty form: beta/h_K * ||J F^-T N|| * (w - 0).v on the listed (cell, local edge) pairs,
 * replaces ElasticModelShapeOpt.penaltyResidual (linear_shell_model.py:323-333) with the
 * ds(100)/dS(100) measures of rm_shell_model.py:88-95.
 * Strong form: zero values on the listed DOFs, replaces dirichletbc/locate_dofs_geometrical
 * (rm_shell_model.py:168-180) as consumed by assembleSystem (fea/utils_dolfinx.py:208-221). */
int femo_set_penalty_facets(femo_ctx* ctx, int32_t nfacets, const int32_t* cell_and_local_edge, double beta);
int femo_set_strong_dofs(femo_ctx* ctx, int32_t n, const int32_t* dofs);

/* Copy an input field into the context (a length-1 array broadcasts) --
 * replaces update(Function, ndarray) (fea/utils_dolfinx.py:319-330).  Besides the six inputs of the model, "dirichlet"
 * (femo_ndof values) sets the prescribed state g of the penalty term beta/h_E |J F^-T N| (w - g).v
 * (linear_shell_model.py:323-333; the reference's RMShellModel always passes zeros, rm_shell_model.py:183-185). */
int femo_set_field(femo_ctx* ctx, const char* name, const double* values, int64_t n);
int femo_get_field(femo_ctx* ctx, const char* name, double* values, int64_t n);

/* Laminated composite law -- the reference's MaterialModelComposite with ElasticModelShapeOpt (linear_shell_model.py:159-190, 268-296).
 * n == 32 * nel enters laminate mode (or replaces its values): per cell, row-major,
 *     [A (3x3), B (3x3), D (3x3), A_s (2x2), c_drill]
 * acting on the Voigt strains eps = (e00, e11, 2 e01), kappa = (k00, k11, 2 k01), gamma = (g0, g1) of the local frame of every
 * quadrature point, E0 = unit(J[:,0]), E1 = E2 x E0 (kinematics.py:54-70).  Frame convention: laminate axis 1 lies along E0, i.e. from
 * vertex 0 toward vertex 1 of the cell as given; reversing a cell's orientation (its normal E2) flips the sign of B.  Through the thickness
 * the strain at height z along E2 is eps - z kappa (u(z) = u_mid - z E2 x theta, linear_shell_model.py:392-398), so a laminate built about
 * its mid-surface has B = -int z Qbar dz (femo_alpha_amd/laminate.py, plies bottom to top along E2).  The energy density is
 * 1/2 (eps.A eps + eps.B kappa + kappa.B eps + kappa.D kappa) + 1/2 gamma.A_s gamma + 1/2 c_drill / h_K^2 omega^2; the operator is its
 * Hessian, so only the symmetric parts act (non-symmetric input is accepted, as in the reference).  Measures as on the isotropic path:
 * membrane, bending and coupling with the strain rule and no J(uhat); shear with the strain rule times J(uhat); drilling with the full
 * rule times J(uhat) (femo_set_strain_quadrature applies).  The reference's drilling coefficient is 12 max(D) over all cells, a constant
 * (the Python layer fills it in); a per-cell c_drill = E h^3 makes a one-ply isotropic laminate reproduce the single-layer law.
 * A reference-plane offset (the mid-surface o above the reference surface) is the host transform A' = A, B' = B - o A,
 * D' = D - o (B + B^T) + o^2 A.
 * Refused with the cell index: non-finite values, a [[A, B], [B, D]] or A_s block whose symmetric part is not positive definite, c_drill <= 0.
 * clt == NULL with n == 0 returns to the single-layer law.  Either way the factor and the Jacobi diagonal are rebuilt before the next solve.
 * In laminate mode:
 *   - "laminate" is an ordinary field (femo_field_size / femo_set_field / femo_get_field), and an argument of femo_dRdarg_T,
 *     femo_total_gradient(s) and femo_dfunctional(ctx, "elastic_energy", "laminate", ...);
 *   - thickness, E, nu and density stay inputs: mass, volume, the compliance regularisation and the von Mises stress outputs (the
 *     reference's ShellStressRM: the single-layer recovery from thickness, E and nu) use them; R does not, so (dR/d thickness|E|nu)^T
 *     lambda is zero.  The strength measure of the plies themselves is "ply_failure" (femo_set_ply_table below);
 *   - the transient operator (femo_set_operator with aM != 0, femo_newmark_*) and the element-partitioned driver (femo_dist_*) are refused. */
int femo_set_laminate(femo_ctx* ctx, const double* clt, int64_t n);
/* Ply failure outputs of a laminate -- new: the reference stops at A / B / D / A_s and has no ply recovery, so this is the project's own
 * contract (pinned by tests/ply_failure_ref.py).  Laminate mode only.  Per cell npt recovery points through the thickness (typically top
 * and bottom of every ply: npt = 2 nply; 1 <= npt <= 32), 16 doubles each, cell-major (n == 16 * npt * nel):
 *     [G (3x3, row-major), z, F1, F2, F11, F22, F66, F12]
 *   - ply-axis stresses at the point: sigma = (s1, s2, t12) = G (eps - z kappa), eps and kappa the Voigt membrane strains and curvatures of
 *     the point's local frame exactly as femo_set_laminate defines them (engineering shear; the strain at height z is eps - z kappa; no
 *     thickness-gradient term: the laminate is constant per cell).  An orthotropic ply has G = Q T(theta), the Q and T of
 *     femo_alpha_amd/laminate.py (ply_stiffness, ply_table);
 *   - failure index FI = F1 s1 + F2 s2 + F11 s1^2 + F22 s2^2 + F66 t12^2 + 2 F12 s1 s2 (Tsai-Wu; Tsai-Hill and von Mises are special
 *     coefficients).  Transverse shear does not enter (its own output is "ply_shear_failure", femo_set_ply_shear_table below).  FI may be negative: nothing takes a root or a non-integer power of it;
 *   - evaluated at the quadrature points of the degree-4 stress measure (3 x 3 Gauss / the 6-point rule), where pnorm_stress is;
 *   - functional "ply_failure" (femo_functional, femo_dfunctional, femo_total_gradient(s)), over the selected sub-domain
 *     (femo_select_subdomain):
 *         K = 1/rho log( 1/(alpha npt) sum_e sum_q w_q det_q J_q(uhat) sum_p exp(rho FI_eqp) )
 *     with alpha the reference area pnorm_stress uses (femo_set_stress_alpha applies; where it is not yet known this value pass
 *     evaluates it itself).  Evaluated with running (max, sum exp(. - max)) pairs: any finite rho FI is safe.  With uhat = 0:
 *     max FI + 1/rho log(min_eq(w det) / (alpha npt)) <= K <= max FI; w = 0 with F1 = F2 = 0 gives K = 0.
 *     femo_dfunctional: wrt "disp_solid" and "ply_table" (16 npt nel, cell-major); zeros for "laminate", "thickness", "E", "nu",
 *     "density", "F_solid".  femo_total_gradient(s): arg "laminate" is -(dR/d laminate)^T lambda, arg "ply_table" the explicit partial
 *     ((dR/d ply_table)^T lambda is zero), "F_solid" as for any functional.  wrt / arg "uhat" is refused: the shape derivative of this
 *     output is not provided.  No float atomics and fixed summation orders: two identical calls return the same bits;
 *   - field femo_ply_failure_field: (nel, npt), entry = max over the cell's quadrature points of FI, every cell whatever the selected
 *     sub-domain (which ply, where -- what a local strength constraint is written in).  Differentiated under the name
 *     "ply_failure_field" in forward mode (femo_field_output_jvp, femo_field_total_jvp) and in reverse (femo_field_output_vjp,
 *     femo_field_output_jacobian, femo_field_total_gradients).  The derivative of an entry is the derivative of FI at the quadrature
 *     point that attains the maximum; on ties the first point in quadrature order wins -- the point the value's running maximum
 *     keeps, which a strict > replaces -- in both modes, which are exact transposes of each other.  It is the one-sided derivative
 *     wherever the maximiser is unique.
 * femo_set_ply_table is refused with the cell index for non-finite entries, and when not in laminate mode, for npt out of range or a
 * wrong n.  table == NULL with n == 0 removes the table; leaving laminate mode removes it too.  The operator does not see the table:
 * the factor and the Jacobi diagonal are kept.  With a table "ply_table" is an ordinary field (femo_field_size / femo_set_field /
 * femo_get_field, npt unchanged).  Without one every call above fails with a message that names femo_set_ply_table.
 * femo_set_ply_failure_params: rho > 0, default 100 (the stress aggregate's default exponent). */
int femo_set_ply_table(femo_ctx* ctx, const double* table, int32_t npt, int64_t n);
int femo_set_ply_failure_params(femo_ctx* ctx, double rho);
int femo_ply_failure_field(femo_ctx* ctx, double* out, int64_t n);

/* Interlaminar (transverse) shear failure outputs of a laminate (femo_alpha_amd/csrc/ply_shear.h) -- new, since FEMO_VERSION 102; the
 * project's own contract like the ply failure outputs (pinned by tests/ply_shear_ref.py).  Laminate mode only.  Per cell npt_s recovery
 * points (1 <= npt_s <= 32), 6 doubles each, cell-major (n == 6 * npt_s * nel):
 *     [Gs (2x2, row-major), F55, F44]
 *   - with q over the degree-4 stress measure (where "ply_failure" is evaluated), wj_eq = w_q det_eq J_eq(uhat) and (ga0, ga1) the
 *     transverse shear strains of the point's local frame as femo_set_laminate defines them:
 *         a_e = sum_q wj_eq,   gbar_e = (1/a_e) sum_q wj_eq (ga0, ga1)_eq,   (t13, t23)_ep = Gs_ep gbar_e,   FI_ep = F55 t13^2 + F44 t23^2.
 *     The index is defined on the CELL-MEAN shear strain: pointwise shear strains of the CG2 x CG1 element are off by tens of per cent
 *     on thin skins where the cell mean reaches the closed form to 1e-9 (README, "Interlaminar shear").  The field is therefore one
 *     smooth number per (cell, point): no maximum over quadrature points, no tie, an unambiguous derivative;
 *   - an orthotropic ply has Gs = diag(G13, G23) R(theta), F55 = 1/S13^2, F44 = 1/S23^2 (femo_alpha_amd/laminate.py: ply_shear_table):
 *     the constitutive first-order-shear recovery, constant within a ply, so one point per ply is enough.  No equilibrium-type
 *     through-thickness profile is built here: callers who want one put their own factors into Gs through the table;
 *   - functional "ply_shear_failure" (femo_functional, femo_dfunctional, femo_total_gradient(s), femo_total_jvp; wherever "ply_failure"
 *     appears, grouped calls included), over the selected sub-domain (femo_select_subdomain):
 *         K = 1/rho log( 1/(alpha npt_s) sum_e a_e sum_p exp(rho FI_ep) )
 *     with the alpha of "ply_failure" (the reference area; femo_set_stress_alpha applies) and its running (max, sum exp) pairs, one slot
 *     per block merged in block order.  With uhat = 0: max FI + 1/rho log(min_e a_e / (alpha npt_s)) <= K <= max FI; w = 0 gives K = 0.
 *     femo_dfunctional: wrt "disp_solid" and "ply_shear_table" (6 npt_s nel, cell-major; zeros outside the selection); exact zeros for
 *     "laminate", "ply_table", "thickness", "E", "nu", "density", "F_solid".  The totals reach "laminate" and "F_solid" through the
 *     adjoint.  wrt / arg "uhat" is refused: the shape derivative of this output is not provided.  For every other output
 *     "ply_shear_table" behaves as "ply_table" does: exact zeros, and (dR/d ply_shear_table)^T lambda = 0;
 *   - field femo_ply_shear_failure_field: (nel, npt_s), entry = FI_ep, every cell whatever the selected sub-domain.  Differentiated in
 *     reverse under the name "ply_shear_failure_field" (femo_field_output_vjp, femo_field_total_gradients: the argument set of
 *     "ply_failure_field" with "ply_shear_table" in place of "ply_table") by the kernels of the aggregate with the cotangent in place of
 *     the KS weight.  femo_field_output_jvp, femo_field_total_jvp and femo_field_output_jacobian(_nnz) refuse the name: not provided.
 * femo_set_ply_shear_table is refused on the host, before any launch, with the cell index for non-finite entries, and when not in
 * laminate mode, for npt out of range or a wrong n; under a layup that carries shear strengths (below) it is refused with a message that
 * names the layup, as femo_set_ply_table is.  table == NULL with n == 0 removes the table; leaving laminate mode removes it too.  The
 * operator does not see the table: the factor and the Jacobi diagonal are kept.  With a table "ply_shear_table" is an ordinary field
 * (femo_field_size / femo_set_field / femo_get_field, npt unchanged).  Without one every call above fails with a message that names
 * femo_set_ply_shear_table.  Every refusal leaves the context unchanged.  femo_set_ply_shear_params: rho finite and > 0, default 100.
 * femo_set_layup_shear_strength (a layup must be active, femo_set_layup below): nply x 2 strengths [S13, S23], finite and > 0, the error
 * names the first offending ply; S == NULL with nply == 0 removes them and the table built from them.  With them the layup owns the
 * shear table: one point per ply (npt_s = nply), rebuilt on the device whenever "ply_angle" is set -- the ply thicknesses do not enter --
 * and "ply_shear_failure" / "ply_shear_failure_field" take the arguments "ply_angle" (per degree, dR/dtheta = [[-n, m], [-m, -n]]) and
 * "ply_thickness" (explicit partial exact zeros; the total comes through the laminate and the adjoint).  The strengths live with the
 * layup as the densities of femo_set_layup_density do: the same nply keeps them, another nply or leaving the mode drops them.
 * The kernels of these outputs use no float atomics and fixed summation orders: two identical calls of femo_functional,
 * femo_dfunctional (every argument, the layup names included), femo_ply_shear_failure_field and femo_field_output_vjp return the same
 * bits.  The guarantee ends where the adjoint solve begins: femo_total_gradient(s), femo_total_jvp and femo_field_total_gradients go
 * through the Krylov refinement of the state operator, whose dot products add their block sums with a float atomic in the order the
 * blocks happen to finish (k_dot, as for every output), so two identical calls agree to the solver's tolerance, not bit for bit; the
 * tangent contractions of femo_total_jvp use the same k_dot.
 * Not provided: the shape derivative; forward mode and the sparse Jacobian of the field; a combined index that adds the shear terms to
 * the in-plane Tsai-Wu index; equilibrium-based through-thickness recovery; per-cell ply materials; the multi-GPU driver; transient
 * laminates; the table-input route of the RMShellModel. */
int femo_set_ply_shear_table(femo_ctx* ctx, const double* table, int32_t npt, int64_t n);
int femo_set_ply_shear_params(femo_ctx* ctx, double rho);
int femo_ply_shear_failure_field(femo_ctx* ctx, double* out, int64_t n);
int femo_set_layup_shear_strength(femo_ctx* ctx, int32_t nply, const double* S);

/* Load-proportional ply strength index (femo_alpha_amd/csrc/ply_strength.h) -- new, since FEMO_VERSION 103; the project's own contract
 * (pinned by tests/ply_strength_ref.py).  The Tsai-Wu index FI = a + b of "ply_failure" has a quadratic part a and a linear part b and
 * is not proportional to the load; the strength ratio (reserve factor) R, the factor by which the load may grow until first-ply failure,
 * is.  These outputs give its inverse r = 1/R, the positive root of a/r^2 + b/r = 1, on the ply table of femo_set_ply_table (or of the
 * layup), unchanged.  At quadrature point q of the degree-4 stress measure and recovery point p, with sigma of "ply_failure":
 *     b = F1 s1 + F2 s2,   a = F11 s1^2 + F22 s2^2 + F66 t12^2 + 2 F12 s1 s2,   D = sqrt(max(b^2 + 4a, 0)),
 *     r = (b + D)/2 for b >= 0,   r = 2a/(D - b) for b < 0,   r = 0 where D = 0;   dr = (r db + da)/D, defined as 0 where D = 0.
 *   r(s w) = s r(w) for s > 0; with F1 = F2 = 0, r = sqrt(FI); scaling the state by 1/r puts FI on 1;
 *   - functional "ply_strength_index" (femo_functional, femo_dfunctional, femo_total_gradient(s) with the sub-domain list, femo_total_jvp,
 *     femo_field_gradient_vec: wherever "ply_failure" appears), over the selected sub-domain:
 *         K = 1/rho log( 1/(alpha npt) sum_e sum_q wj_eq sum_p exp(rho r_eqp) )
 *     with the wj, alpha and rho of "ply_failure" (femo_set_ply_failure_params: both indices are of order one at failure).  With
 *     uhat = 0: max r + 1/rho log(min wj / (alpha npt)) <= K <= max r; w = 0 gives K = 0 with the reference area, and exactly zero
 *     gradients.  femo_dfunctional: wrt "disp_solid" and "ply_table" from the kernels; exact zeros for "laminate", "thickness", "E",
 *     "nu", "density", "F_solid", "ply_shear_table"; "ply_thickness" / "ply_angle" through the layup's pull-back; "uhat" is refused: the
 *     shape derivative of this output is not provided;
 *   - field femo_ply_strength_index_field: (nel, npt), entry = max_q r_eqp, every cell whatever the selection; the first maximiser in
 *     quadrature order wins and a NaN stays visible.  Differentiated in reverse at that maximiser under the name
 *     "ply_strength_index_field" (femo_field_output_vjp, femo_field_total_gradients; the argument set of "ply_failure_field", cotangents
 *     grouped four to a solve).  femo_field_output_jvp, femo_field_total_jvp and femo_field_output_jacobian(_nnz) refuse the name: not
 *     provided.
 * r needs a >= 0: the quadratic form of every recovery point must be positive semidefinite, F11, F22, F66 >= 0 and
 * F12^2 <= F11 F22 (1 + 1e-12) (the slack covers the rounding of tsai_wu(f12 = +-1)).  The table is checked on the device at most once
 * per upload or femo_set_layup, when one of these outputs is first asked for; a failing table is refused with an error that names the
 * cell and the point, and "ply_failure" keeps working on it.  The outputs keep their own block slots and results: a call never
 * disturbs the shift the gradients of "ply_failure" read.  No float atomics and fixed summation orders: two identical calls of
 * femo_functional, femo_dfunctional, femo_ply_strength_index_field and femo_field_output_vjp return the same bits; the totals repeat to
 * the solver's tolerance, as for the shear outputs above.
 * Not provided: the shape derivative; forward mode and the sparse Jacobian of the field; a ratio for the shear index (it is
 * sqrt(FI), the caller's one line); transient laminates; the multi-GPU driver. */
int femo_ply_strength_index_field(femo_ctx* ctx, double* out, int64_t n);

/* Hashin fibre and matrix failure indices (femo_alpha_amd/csrc/ply_hashin.h) -- new, since FEMO_VERSION 104; the project's own contract
 * (pinned by tests/ply_hashin_ref.py).  The criteria above are single polynomials on the ply table and cannot tell which mode is
 * critical; Hashin's (1980) separates fibre from matrix failure and switches its formula on the sign of a stress component, which no
 * table of quadratic forms can express.  With sigma = (s1, s2, t12) = G (eps - z kappa) of "ply_failure" (entries 0..9 of the ply
 * table of femo_set_ply_table or of the layup; entries 10..15 are not read) and six strengths [Xt, Xc, Yt, Yc, SL, ST] per (cell,
 * recovery point), all finite and > 0:
 *     fibre   FI_f = (s1/Xt)^2                              s1 >= 0        FI_f = (s1/Xc)^2                          s1 < 0
 *     matrix  FI_m = (s2/Yt)^2 + (t12/SL)^2                 s2 >= 0        FI_m = (s2/(2 ST))^2 + c1 s2 + (t12/SL)^2   s2 < 0,
 *     c1 = ((Yc/(2 ST))^2 - 1)/Yc.
 * Hashin's shear term in fibre tension (his alpha) is taken as 0: FI_f is C1 and sqrt(FI_f) is proportional to the load.  FI_m is
 * continuous with a derivative kink at s2 = 0 unless ST = Yc/2, may be negative, and is differentiated on the branch of the sign;
 * s1 = 0 and s2 = 0 take the tension branch; a NaN passes through.
 *   - femo_set_ply_hashin_table: table is (nel, npt, 6) cell-major in solver cell order; NULL with n = 0 removes it.  Laminate mode
 *     only; the factor is kept.  The strengths are checked on the device once per upload; a refusal names the entry, the recovery
 *     point and the cell, and the table the context held stays.  npt must equal the ply table's when an output is asked for.  Leaving
 *     laminate mode, and a femo_set_layup with another number of recovery points, drop the table.
 *   - functionals "ply_hashin_fibre" and "ply_hashin_matrix" (femo_functional, femo_dfunctional, femo_total_gradient(s) with the
 *     sub-domain list, femo_total_jvp), over the selected sub-domain:
 *         K = 1/rho log( 1/(alpha npt) sum_e sum_q wj_eq sum_p exp(rho FI_eqp) )
 *     with the wj, alpha and rho of "ply_failure" (femo_set_ply_failure_params).  femo_dfunctional: wrt "disp_solid" and "ply_table"
 *     from the kernels (columns 10..15 of the table gradient are exact zeros; zeros outside the selection); exact zeros for
 *     "laminate", "thickness", "E", "nu", "density", "F_solid", "ply_shear_table"; "ply_thickness" / "ply_angle" through the layup's
 *     pull-back; "uhat" is refused: the shape derivative of these outputs is not provided;
 *   - fields femo_ply_hashin_field: (nel, npt) each, entry = max_q FI_eqp, every cell whatever the selection, both computed in one
 *     pass; either pointer may be NULL.  The first maximiser in quadrature order wins and a NaN stays visible.  Differentiated in
 *     reverse at that maximiser under the names "ply_hashin_fibre_field" and "ply_hashin_matrix_field" (femo_field_output_vjp,
 *     femo_field_total_gradients; the argument set of "ply_strength_index_field").  femo_field_output_jvp, femo_field_total_jvp and
 *     femo_field_output_jacobian(_nnz) refuse the names: not provided.
 * The outputs keep block slots and results of their own per index: a call never disturbs the other ply outputs.  No float atomics and
 * fixed summation orders: two identical calls return the same bits; the totals repeat to the solver's tolerance.
 * Not provided: Hashin's alpha > 0; derivatives with respect to the strengths; the shape derivative; forward mode and the sparse
 * Jacobian of the fields; a combined index over both modes (take the max, or constrain both); transient laminates; the multi-GPU
 * driver. */
int femo_set_ply_hashin_table(femo_ctx* ctx, const double* table, int32_t npt, int64_t n);
int femo_ply_hashin_field(femo_ctx* ctx, double* fibre, double* matrix, int64_t n);

/* Layups: the laminate and the ply table built on the device from the design variables of a laminate, ply thicknesses and ply angles
 * (femo_alpha_amd/csrc/layup.h) -- new; the conventions are those of femo_alpha_amd/laminate.py (clt_from_plies, ply_table):
 *   - nply plies (1..32), listed bottom to top along the cell normal, the same materials in every cell: plies is nply x 12,
 *     [E1, E2, G12, nu12, G13, G23, F1, F2, F11, F22, F66, F12] (F*: the Tsai-Wu coefficients of laminate.tsai_wu);
 *   - t and theta: nel x nply, cell-major; interfaces z_i = sum_{j<i} t_j - H / 2 about the mid-surface, the default reference surface
 *     (femo_set_layup_reference below chooses another); angles in degrees from E0 toward E1;
 *   - A = sum (z1 - z0) Qbar, B = -1/2 sum (z1^2 - z0^2) Qbar, D = 1/3 sum (z1^3 - z0^3) Qbar, A_s = 0.833 sum t Qsbar, and
 *     c_drill (> 0), a constant of the mode that every derivative holds fixed;
 *   - surfaces: a mask of 1 (bot), 2 (mid), 4 (top) of every ply; the recovery points run ply by ply from the bottom, inside a ply in
 *     the order bot, mid, top, G = Q T(theta); nply x popcount(surfaces) <= 32.  0: no recovery points -- no ply table, and
 *     "ply_failure" answers as it does without one.
 * femo_set_layup enters laminate mode if needed (transient operators are refused as by femo_set_laminate).  The per-ply constants are
 * checked on the host (finite, moduli > 0, 1 - nu12^2 E2 / E1 > 0), t > 0 and finite values on the device: the error names the first
 * offending cell and ply.  A refused call changes nothing.  Valid plies give a positive definite laminate, so no block is factorised.
 * While a layup is active:
 *   - "ply_thickness" and "ply_angle" are fields of nel x nply values (femo_field_size, femo_set_field, femo_get_field; cell-major);
 *     setting either rebuilds the laminate and the table on the stream, and the next solve re-factorises.  femo_device_ptr returns the
 *     device copies, which are ply-major ([k][nel]).  Outside the mode both names are unknown (femo_field_size: -1);
 *   - femo_get_field "laminate" / "ply_table" return what was built (symmetric blocks); femo_set_laminate with values, femo_set_ply_table
 *     and femo_set_field of "laminate" / "ply_table" are refused with a message that names femo_set_layup;
 *   - both names are arguments of femo_dfunctional, femo_dRdarg_T, femo_residual_jvp, femo_total_gradient(s) and femo_total_jvp, by
 *     d/dx = (d laminate/dx)^T [d/d laminate] + (d table/dx)^T [d/d ply_table] (or its forward counterpart), composed on the device.
 *     Angle derivatives are per degree;
 *   - both names are arguments of femo_field_output_vjp and femo_field_total_gradients for the field "ply_failure_field" (below);
 *   - not provided: every other derivative of the field outputs with respect to the layup (the stress fields in femo_field_output_vjp
 *     and femo_field_total_gradients, and every field in femo_field_output_jvp, femo_field_output_jacobian, femo_field_total_jvp,
 *     femo_field_gradient_vec and femo_dist_gradient refuse both names), the regularisation
 *     from the layup (it keeps the "thickness" field, as "mass" and "volume" keep "thickness" and "density"), per-cell ply
 *     materials, the multi-GPU driver and transient laminates.
 * Mass and volume from the layup (femo_alpha_amd/csrc/layup_mass.h) -- new: two functionals of the layup itself, over the selected
 * sub-domain (femo_select_subdomain; "mass" and "volume" integrate the whole mesh), on the quadrature tables "mass" uses:
 *     "layup_mass"   = sum_e (sum_k rho_k t_ek) sum_q w_q det_q J_q(uhat)
 *     "layup_volume" = sum_e (sum_k t_ek)       sum_q w_q det_q J_q(uhat)
 *   - femo_set_layup_density: nply densities rho_k, the same in every cell like the other per-ply constants.  A layup must be active
 *     and nply must be its ply count; values finite and >= 0, the error names the first offending ply; rho == NULL with nply == 0
 *     removes them.  A refused call changes nothing.  The densities live with the layup: a later femo_set_layup with the same nply
 *     and femo_set_field of "ply_thickness" / "ply_angle" keep them, another nply drops them, leaving the mode drops them.  The
 *     operator does not see them: the factor and the Jacobi diagonal are kept;
 *   - "layup_mass" without densities fails with a message that names femo_set_layup_density; "layup_volume" needs none.  Outside a
 *     layup both names are unknown functionals;
 *   - femo_dfunctional: wrt "ply_thickness" is rho_k (or 1) times the cell's integrated w det J, zero outside the selection; wrt
 *     "uhat" the shape derivative; exact zeros for "ply_angle", "disp_solid", "laminate", "ply_table", "thickness", "E", "nu",
 *     "density" and "F_solid".  These outputs see the layup directly, never through the laminate;
 *   - femo_total_gradient(s) and femo_total_jvp accept both names with every argument: neither depends on the state, so the total is
 *     the explicit partial, a call that names only these outputs solves and factorises nothing and reports iters = 0, relres = 0
 *     (femo_total_jvp: unless dW is asked for), and in a grouped call their columns stay out of the grouped sweeps;
 *   - the value and the thickness gradient use no atomics and fixed summation orders: two identical calls return the same bits.  The
 *     shape derivative accumulates on the vertices with the atomics of the other outputs' shape derivatives.
 * The reference surface of the layup (femo_set_layup_reference) -- new: the surface the mesh stands for, and about which the laminate
 * and the z of the table are built.  It is given by a number r, its position below the mid-surface in units of the cell's total
 * thickness H_e (0: the mid-surface, 1/2: the bottom, -1/2: the top; any finite value), and an optional length c_e per cell:
 *     o_e = r H_e + c_e                               how far the reference surface lies below the mid-surface
 *     z_i = sum_{j<i} t_j - (1/2 - r) H_e + c_e       bottom: z_0 = c_e, top: z_nply = c_e
 *     d z_i / d t_j = [j < i] - (1/2 - r)             c_e is data, not an argument
 *   - A, B, D and column 9 of the table follow from these z_i as above; A, A_s, G, the strength coefficients, the shear table,
 *     "layup_mass" and "layup_volume" do not see the reference surface.  A symmetric stack about its bottom or top has B != 0.  One
 *     isotropic ply about its bottom gives A = h C, B = -h^2 / 2 C, D = h^3 / 3 C, the reference's single layer with BOT;
 *   - offset: n == nel values, n == 1 (the same in every cell), or NULL / 0 (none).  A layup must be active, r and every offset finite
 *     (the error names the first offending cell; a length error names both lengths).  A refused call changes nothing;
 *   - an accepted call rebuilds the laminate and the table and counts as a change of the operator, as a new "ply_thickness" does: the
 *     next solve re-factorises.  c_drill is a constant of the mode and stays;
 *   - the reference surface belongs to the mode, not to the plies: femo_set_field of "ply_thickness" / "ply_angle" and a further
 *     femo_set_layup, of any ply count, keep it; leaving the mode (either way below) returns to the mid-surface;
 *   - femo_layup_jvp / femo_layup_vjp and every derivative entry point that reaches the layup differentiate about the chosen surface,
 *     for both arguments; r = 0 without offsets performs the operations of the mid-surface convention, bit for bit;
 *   - femo_get_layup_reference: r, and the nel offsets (zeros where none were given); either pointer may be NULL;
 *   - not provided: the offset as a differentiable argument, and a reference surface outside the layup mode.
 * femo_set_layup(ctx, 0, NULL, 0, 0, NULL, NULL) leaves the mode and keeps the last laminate and table as ordinary values;
 * femo_set_laminate(ctx, NULL, 0) drops the layup together with the laminate.
 * femo_layup_jvp: ndir directions V (ndir x n, n = nel nply) -> dlaminate (ndir x 32 nel) and dtable (ndir x 16 npt nel); either may be
 * NULL.  femo_layup_vjp: out (n) = J^T (laminate_bar, table_bar); either may be NULL.  One thread per cell and no atomics: two identical
 * calls return the same bits. */
int femo_set_layup(femo_ctx* ctx, int32_t nply, const double* plies, int32_t surfaces, double c_drill, const double* t, const double* theta);
int femo_set_layup_density(femo_ctx* ctx, int32_t nply, const double* rho);
int femo_set_layup_reference(femo_ctx* ctx, double r, const double* offset, int64_t n);
int femo_get_layup_reference(femo_ctx* ctx, double* r, double* offset, int64_t n);
int femo_layup_jvp(femo_ctx* ctx, const char* wrt, int32_t ndir, const double* V, int64_t n, double* dlaminate, double* dtable);
int femo_layup_vjp(femo_ctx* ctx, const char* wrt, const double* laminate_bar, const double* table_bar, double* out, int64_t n);

/* State access -- replaces getFuncArray / setFuncArray on the state Function
 * (fea/utils_dolfinx.py:174-186). */
int femo_set_state(femo_ctx* ctx, const double* w);
int femo_get_state(femo_ctx* ctx, double* w);

/* y = (dR/dw) x, matrix-free, element by element (elastic energy Hessian + penalty, strong-BC rows
 * replaced by identity) -- replaces assembleMatrix(dR_du) followed by a mat-vec
 * (csdl_alpha_opt/state_operation.py:289; fea/utils_dolfinx.py:275-283). */
int femo_apply_K(femo_ctx* ctx, const double* x, double* y);
/* r = R(w) for the current fields (w == NULL: the stored state) -- replaces
 * assemble_vector(form(residual_form)) (fea/utils_dolfinx.py:194-198; linear_shell_model.py:308-321). */
int femo_residual(femo_ctx* ctx, const double* w, double* r);
/* F = int f . v J dx, the load part of the residual (linear_shell_model.py:320). */
int femo_load_vector(femo_ctx* ctx, double* F);
/* Diagonal of the operator femo_apply_K applies (the Jacobi preconditioner). */
int femo_diagonal(femo_ctx* ctx, double* d);
/* Dense element matrices K_e, nel*ldof*ldof, element-local order [u_a xyz ..., theta_b xyz ...]
 * (what FFCx's tabulate_tensor produces for derivative(residual, w)). */
int femo_element_matrices(femo_ctx* ctx, int32_t first, int32_t count, double* Ke);

/* Multifrontal Cholesky preconditioner: upload the symbolic analysis (elimination tree of a nested
 * dissection of the elements, fronts, index maps -- femo_alpha_amd/solver/symbolic.py).  Plays the part
 * of MUMPS' analysis phase behind setUpKSP_MUMPS (fea/utils_dolfinx.py:514-531).  Arrays: per tree node
 * nf, npiv, parent, left, right; front_off (ntree+1, doubles), dof_off (ntree+1); front_dofs / up_map
 * (dof_off[ntree] entries); level_off (nlevels+1) into level_nodes (ntree, children before parents);
 * elem_front (nel) and elem_map (nel*ldof) place every element matrix in its leaf front. */
int femo_set_frontal_plan(femo_ctx* ctx, int32_t ntree, int32_t nlevels, const int32_t* nf, const int32_t* npiv,
                          const int64_t* front_off, const int64_t* dof_off, const int32_t* front_dofs,
                          const int32_t* up_map, const int32_t* parent, const int32_t* left, const int32_t* right,
                          const int32_t* level_off, const int32_t* level_nodes, const int32_t* elem_front,
                          const int32_t* elem_map);
/* Numeric factorisation for the current fields (also run lazily by the solves when preconditioner == 2):
 * element matrices -> leaf fronts -> batched partial Cholesky level by level.  Replaces ksp.setUp() with
 * PC 'lu' / MUMPS (fea/utils_dolfinx.py:495-531). */
int femo_factorize(femo_ctx* ctx);
/* One factorisation with a HIP event pair around every launch; per kernel class (0 rows below the diagonal blocks,
 * 1 diagonal blocks, 2 trailing rank-k updates, 3 extend_add, 4 front_assemble, 5 memset, 6 inversion of L11, 7 unused):
 * out32[0..7] total ms, out32[8..15] launches, out32[16..23] algorithmic flops (lower triangles only) executed by the
 * launches of the class -- counted from each launch's own K and column ranges -- and out32[24..31] their compulsory HBM
 * bytes (every operand entry read once, results read and written once); classes 0, 1, 2, zero otherwise. */
int femo_factorize_profile(femo_ctx* ctx, double* out32);
/* One application of the factor (forward + backward sweep) with HIP events between the launches, per tree level L:
 * out[4 L + 0 / 1] forward sweep, first / second launch; out[4 L + 2 / 3] backward sweep (ms); n >= 4 * levels. */
int femo_sweep_profile(femo_ctx* ctx, double* out, int64_t n);
/* ... and of the sweeps with nrhs = 2 or 4 interleaved vectors (femo_solve_linear_multi): out[2 L] forward, out[2 L + 1] backward sweep of
 * level L in ms; n >= 2 nlevels. */
int femo_sweep_profile_multi(femo_ctx* ctx, int32_t nrhs, double* out, int64_t n);
/* out6: [0] front assembly ms, [1] factorisation ms, [2] front storage GB, [3] factor GFLOP,
 *       [4] non-positive pivots repaired, [5] number of fronts. */
int femo_frontal_info(const femo_ctx* ctx, double* out6);

/* Solver configuration. preconditioner: 0 = Jacobi, 2 = multifrontal Cholesky (needs a frontal plan).
 * check_every: convergence is polled on the host every this many PCG iterations. */
int femo_set_solver(femo_ctx* ctx, int preconditioner, double rtol, int32_t maxit, int32_t check_every);
/* Schedule switches and failure policy of the solvers (they are per context; nothing is read from the environment):
 *   "strict" (default 1)             a Krylov solve that reaches maxit short of rtol returns 4 with a message -- the reference
 *                                    solves with a direct LU (fea/utils_dolfinx.py:466,514-531), an unconverged state has no
 *                                    counterpart there; 0 returns 0 and leaves the judgement to iters / relres
 *   "allow_pivot_repair" (default 0) 0: a non-positive pivot makes femo_factorize (and the solves that call it) return 5;
 *                                    1: such pivots are replaced and counted (femo_frontal_info [4])
 *   "trailing" 0 auto | 1 left-looking | 2 right-looking rank-k updates; "left_min", "left_max" (auto: levels with this
 *   many fronts are left-looking; defaults 64, 2048); "super_panel" (default 512; 0 = off), "super_panel_cnt" (default 64):
 *   right-looking levels of at most that many fronts update the trailing matrix once per super-panel of that many factor
 *   columns instead of once per 128; "lookahead" 0/1, "lookahead_cnt": levels of fewer fronts than that on the 128-column
 *   schedule run the bulk of an update on a second stream beside the next panel;
 *   "fused_schur" (default 1): Schur complements are gathered from the children by the rank-k update that touches them
 *   first instead of by the extend-add;
 *   "gather_mono" (default 1): the kernels that gather a front from its children's Schur complements address a front whose
 *   two children land in increasing rows (every front of the package's default plan) per column, without ordering each pair of
 *   child rows; 0: the general gather everywhere.  The factor is the same bit for bit;
 *   "fuse_rows" (default 1), "fuse_rows_cnt" (2048), "fuse_rows_np" (256): levels of at least that many fronts whose widest front has at most
 *   that many pivots form the rows under a diagonal block inside the diagonal-block kernel;
 *   "rows_fine_wg" (96), "narrow_fine_wg" (128): launches of at most that many workgroups take the kernels with 16 rows / a 16 x 16 block per wave;
 *   "stale_factor" (default 0)       n > 0: when only FIELDS (thickness, E, nu, density, uhat) changed since the last factorisation, that
 *                                    factor is kept as the PCG preconditioner and the operator is re-factorised only if a solve has not
 *                                    converged after n iterations (the iteration then restarts from the iterate it reached), and at once
 *                                    if a field has moved more than "stale_rel" (default 2e-3, relative L2 norm) from the factor's design:
 *                                    beyond that the extra iterations cost more than the factorisation (profiles/r5_stale_factor.txt).  PCG works on
 *                                    the current matrix-free operator: the solution is the same.  For optimisation loops, where successive
 *                                    designs are close; the reference itself never refreshes its derivative matrices
 *                                    (csdl_alpha_opt/state_operation.py:130-131).  femo_last_timing [3] says which factor a solve used;
 *   "apply_lanes" (0): 5 = the matrix-free operator with five lanes per element instead of a quad of lanes -- measured slower, off
 *   (profiles/r6_apply_lanes.txt); "sweep_ahead" (2), "multi_rhs" (1): DESIGN.md section 0;
 *   "assemble_fc" (1): front assembly with one workgroup per leaf front -- zero fill, element columns and their sums without float
 *   atomics, the front written once (k_front_assemble_fc).  1: where it was measured to pay (triangles and CG1CG1, or at least 20
 *   quadrature points per cell), 2: always, 0: never = one wave per element adding with atomics into zero-filled fronts
 *   (profiles/r5_assemble_fc_ab.txt);
 *   "sweep_w" (0): W = L21 L11^-1 stored where L21 was, a wide level of a sweep as one launch instead of two -- an application 4 % shorter,
 *   the factorisation 1.5 ms longer, off (profiles/r5_sweep_w_ab.txt); changing it discards the factor;
 *   "equilibrate" (0), "precond_nquad" (0): measured experiments, off;
 *   "grid_chunk" (fronts per launch, <= 65535);
 *   "wide_np", "wide_cnt" (which tree levels take the wide triangular-solve kernels; before femo_set_frontal_plan);
 *   "swork_slots" (default 8192; before femo_set_frontal_plan): 128 x 128 scratch blocks for the diagonal-block inverses of
 *   the levels solved with one workgroup per front -- levels with more fronts are factorised in chunks of that many;
 *   "bnd_tiled_nb" (backward sweep: levels whose largest boundary block has at least this many rows use 128 x 128 tiles
 *   with atomics for L21^T x, the others one workgroup per 16 columns); "profile_verbose" (per-launch timings of
 *   femo_factorize_profile on stderr). */
int femo_set_option(femo_ctx* ctx, const char* key, double value);
/* Krylov method for the state / adjoint / linear solves: 0 = conjugate gradients (default; the operator is SPD),
 * 1 = right-preconditioned BiCGStab with the same preconditioner (femo_set_solver).  Stands where the reference
 * chooses its PETSc KSP type (fea/utils_dolfinx.py:495-531). */
int femo_set_krylov(femo_ctx* ctx, int method);

/* Forward solve R(w) = 0 for the current fields, result kept on the device as the state.
 * Replaces FEA.solve -> solveNonlinear -> NewtonSolver + MUMPS LU (fea/fea_dolfinx.py:159-170,
 * fea/utils_dolfinx.py:338-352,438-468): the residual is linear in w, so one PCG solve of
 * K w = F reproduces what the reference's three Newton iterations converge to.
 * zero_guess != 0 starts from w = 0, otherwise from the stored state (the reference keeps the
 * previous solution as initial guess, fea_dolfinx.py:45,165). */
int femo_solve_state(femo_ctx* ctx, int zero_guess, int32_t* iters, double* relres);
/* x = K^-1 rhs with BC rows of x zeroed afterwards -- replaces FEA.solveLinearBwd / solveLinearFwd
 * (fea/fea_dolfinx.py:173-203) and the BC zeroing of state_operation.py:216-218.  K is symmetric, so
 * the same call serves both modes (reference quirk Q3). */
int femo_solve_linear(femo_ctx* ctx, const double* rhs, double* x, int32_t* iters, double* relres);
/* Several right-hand sides at once: rhs and x hold nrhs vectors of femo_ndof entries, one after the other; iters / relres: nrhs entries
 * (or NULL).  With the multifrontal preconditioner (femo_set_solver preconditioner 2) the right-hand sides go through the triangular
 * sweeps in groups of up to four with the vectors interleaved, so that the factor is read once per group instead of once per vector
 * (option "multi_rhs" 0: one at a time); every right-hand side keeps its own PCG recurrence and stopping test, so the iterates are those
 * of nrhs separate femo_solve_linear calls.  Replaces repeated StateOperation.apply_inverse_jacobian calls (state_operation.py:188-220),
 * forward or reverse (K is symmetric).  Status 4 if any right-hand side stops at maxit short of rtol (option "strict"). */
int femo_solve_linear_multi(femo_ctx* ctx, int32_t nrhs, const double* rhs, double* x, int32_t* iters, double* relres);
/* One application of the multifrontal preconditioner, no Krylov iteration: out_r = M^-1 in_r for nrhs host vectors of femo_ndof entries,
 * one after the other, with M = L L^T the current factorisation (made first if there is none; femo_enable_frontal's plan needed).  The
 * route is that of the PCG loop: one vector through the context's own sweep (the captured graph of option "sweep_graph", the scaling of
 * option "equilibrate"); several, when the grouped solves apply, in groups of up to four interleaved vectors as femo_solve_linear_multi
 * sweeps them.  For checking the factor itself: PCG corrects any error of M^-1, this call does not. */
int femo_frontal_apply(femo_ctx* ctx, int32_t nrhs, const double* in, double* out);

/* pressure = A^-1 force with A the consistent mass matrix of the pressure space [CG1]^3 (node-major xyz, 3 nn entries) -- replaces
 * csdl.solve_linear(A, force) on the matrix of RMShellPDE.construct_force_to_pressure_map (rm_shell/rm_shell_model.py:414-421,
 * rm_shell_pde.py:194-209; dynamic_rm_shell/plate_sim.py:452-468).  Jacobi-preconditioned conjugate gradients with the matrix
 * applied cell by cell on the device; A is symmetric, so the same call serves the reverse mode.  Status 4: maxit reached short of
 * rtol (option "strict"). */
int femo_force_to_pressure(femo_ctx* ctx, const double* force, double* pressure, double rtol, int32_t maxit, int32_t* iters, double* relres);

/* ---- Dynamic shell (reference femo_alpha/dynamic_rm_shell/plate_sim.py:131-140,190-215): building blocks on
 * device vectors.  The time loop and its adjoint live in femo_alpha_amd/dynamic_rm_shell (Python, like the
 * reference's PlateSim); these calls supply the operator A = aK K + aM M of one midpoint/Newmark step, its
 * factorisation and solves, the reduced strain quadrature, and the thickness-gradient pieces. */
int femo_set_operator(femo_ctx* ctx, double aK, double aM);          /* operator used by solves and femo_factorize */
int femo_set_strain_quadrature(femo_ctx* ctx, int32_t nred);         /* nred x nred Gauss for membrane/bending/shear; 0 = full rule */
/* The rule of the static forms after creation -- same meaning as femo_create's nquad (ShellElement.getQuadratureRule with given
 * degrees, linear_shell_model.py:88-103).  Factor and Jacobi diagonal of the old rule are dropped.  femo_get_quadrature: the rule in
 * use and its number of points per cell. */
int femo_set_quadrature(femo_ctx* ctx, int32_t nquad);
int femo_get_quadrature(femo_ctx* ctx, int32_t* nquad, int32_t* npoints);
/* Host only, no device needed: the quadrature and shape tables of a rule exactly as the kernels receive them (what basix tabulates for
 * the reference, linear_shell_model.py:47-103), so that a caller or a test can compare them bit for bit with its own.  Arrays hold 36
 * points: w, wS [36]; N2 [36][9]; dN2 [36][9][2]; N1, NR [36][4]; dN1, dNR [36][4][2]; any pointer may be NULL. */
int femo_quadrature_tables(int32_t nvc, int32_t nquad, int32_t nred, int32_t cg1, int32_t cr, int32_t* npoints, double* w, double* wS,
                           double* N2, double* dN2, double* N1, double* dN1, double* NR, double* dNR);
int femo_op_apply_vec2(femo_ctx* ctx, int32_t src, int32_t dst, double aK, double aM, int with_penalty);
int femo_solve_vec(femo_ctx* ctx, int32_t b, int32_t x, int zero_guess, int32_t* iters, double* relres);
int femo_vec_mask_zero(femo_ctx* ctx, int32_t id);
int femo_grad_reset(femo_ctx* ctx);                                   /* thickness-gradient accumulator := 0 */
int femo_grad_add(femo_ctx* ctx, int kind, int32_t x, int32_t y, double scale);   /* += scale y^T dK/dh x (0) or y^T dM/dh x (1) */
int femo_grad_get(femo_ctx* ctx, double* out, int64_t n);

/* ---- CSR assembly of the elastic stiffness matrix (what assembleMatrix(dR_du) hands back in the reference,
 * csdl_alpha_opt/state_operation.py:289, fea/utils_dolfinx.py:200-206).  The solver never needs it (the operator is
 * matrix-free); it exists for callers that want the matrix.  The map -- the nel*ldof^2 element contributions sorted by CSR
 * destination -- and the pattern are built on the device by femo_build_csr_map (once per mesh; what dolfinx create_matrix does
 * per form); femo_set_csr_map accepts a map built elsewhere (femo_alpha_amd/csr.py, the host cross-check).
 * ms2 = { element matrices ms, scatter ms }. */
int femo_build_csr_map(femo_ctx* ctx, int32_t* nnz);
int femo_get_csr_pattern(femo_ctx* ctx, int32_t* rowptr, int32_t* colidx);
int femo_set_csr_map(femo_ctx* ctx, int32_t nnz, int64_t ncontrib, const int32_t* perm, const int32_t* dest);
int femo_assemble_csr(femo_ctx* ctx, double* vals, double* ms2);

/* Stress aggregation parameters (m, rho) of pnorm_stress = 1/alpha int (m vm_top)^rho J dx
 * (rm_shell/rm_shell_pde.py:112-128; defaults 1e-6, 100 as rm_shell_model.py:63). */
int femo_set_stress_params(femo_ctx* ctx, double m, double rho);
/* alpha of the aggregate given by the caller (pnorm_stress(alpha=...), rm_shell_pde.py:123-127) for the whole mesh (sel = -1) or a
 * sub-domain; alpha <= 0: back to the reference area evaluated at first use. */
int femo_set_stress_alpha(femo_ctx* ctx, int32_t sel, double alpha);
/* Sub-domains for the stress aggregate -- the reference's mesh tags / dxx(i) measure
 * (rm_shell/rm_shell_model.py:101-133, 242-253).  tags[nel] holds the sub-domain index of every cell
 * (0 .. ntags-1, or -1 for none).  femo_select_subdomain(sel) restricts "pnorm_stress" and its derivatives to the
 * cells of sub-domain sel, normalised by that sub-domain's reference area; sel = -1 selects the whole mesh again. */
int femo_set_cell_tags(femo_ctx* ctx, const int32_t* tags, int64_t n, int32_t ntags);
int femo_select_subdomain(femo_ctx* ctx, int32_t sel);
/* Max-displacement aggregates of the static state (femo_alpha_amd/csrc/disp_aggregate.h) -- new: the smooth maximum the reference's
 * static sizing examples build on the host, tip_displacement = csdl.maximum(csdl.norm(disp_extracted, axes=(1,)))
 * (ex_lpc_shell_w_caddee.py:752, ex_tiltrotor_shell.py:398), as functionals of the library.  The contract is the project's own
 * (csdl_alpha's maximum / norm are not checked against it); tests/disp_aggregate_ref.py restates it.
 *   - displacement nodes are the nodes whose three translations are w[3 i .. 3 i + 2]: the P2 nodes, the mesh vertices being the first
 *     nn of them.  A node is selected when it belongs to at least one cell of the selected sub-domain (femo_select_subdomain; -1: every
 *     cell) and its kind is asked for: nodes = 0 the mesh vertices only (what disp_extracted holds), nodes = 1 every displacement node
 *     (the same set on CG1CG1).  N is the number of selected nodes;
 *   - four parameter slots, so that several constraints (an upper limit, a lower limit, a magnitude) share one grouped adjoint call:
 *     the functionals "max_disp" (slot 0), "max_disp1", "max_disp2", "max_disp3".  Per slot rho > 0, a scaler s, an optional direction
 *     d (3 values, used as given, not normalised) and nodes; before any call rho = 100, s = 1, no direction, nodes = 0;
 *   - norm mode (no direction): x_i = s |u_i|, s > 0, |u| the plain sqrt(ux^2 + uy^2 + uz^2).  Direction mode: x_i = s (d . u_i),
 *     s != 0; s < 0 gives a smooth minimum of d . u;
 *   - S = x_max + (1/rho) log sum_i exp(rho (x_i - x_max)) and M = S / s: every exponent is <= 0, any finite rho x is safe;
 *     p_i = exp(rho (x_i - S)), sum_i p_i = 1; dM/du_i = p_i u_i / |u_i| in norm mode (exactly 0 where |u_i| = 0, a subgradient as for
 *     "pnorm_stress" at zero stress) and p_i d in direction mode; rotations and unselected nodes get exact zeros;
 *   - bounds: s > 0: max_i x_i / s <= M <= max_i x_i / s + log N / (rho s);  s < 0: min_i d.u_i - log N / (rho |s|) <= M <= min_i d.u_i.
 *     With w = 0 in norm mode M = log N / (rho s) and the gradient is all zeros;
 *   - M does not depend on uhat, thickness, E, nu, density, F_solid, the laminate, the ply table or the layup (nodal values are not
 *     integrals): femo_dfunctional gives exact zeros for these arguments (the layup names through the composition) and refuses unknown
 *     arguments as for every functional;
 *   - the four names are legal in femo_functional, femo_dfunctional, femo_dfunctional_vec, femo_total_gradient(s) and femo_total_jvp, in
 *     any mix with the other functionals; subdomains[i] applies per functional;
 *   - femo_set_disp_aggregate refuses, changing nothing: a slot outside 0..3, rho <= 0 or not finite, a scaler that is zero or not
 *     finite, a scaler < 0 without a direction, a direction that is zero or not finite, nodes not 0 or 1.  direction = NULL: norm mode.
 *     The operator does not see these parameters: the factor and the Jacobi diagonal are kept;
 *   - errors: a selection without nodes (N = 0; the message names the sub-domain); a non-finite translation at a selected node (the
 *     value call fails with a message); not provided, with that wording: a context with ghost entries (femo_create_ghost /
 *     femo_create_element with nghost > 0) and a context after femo_dist_setup, where replicated separator nodes would be counted once
 *     per partition;
 *   - no float atomics: block results are merged in a fixed order, and the value, the gradient and the grouped totals of two identical
 *     calls have the same bits.  The node mask of a selection is built at first use and kept until femo_set_cell_tags; results do not
 *     depend on whether it was kept.  The state, the fields and the factor are never written. */
int femo_set_disp_aggregate(femo_ctx* ctx, int32_t slot, double rho, double scaler, const double* direction, int32_t nodes);
/* Field outputs "stress" (top surface, xi2 = h/2), "stress_mid" (xi2 = 0), "stress_bot" (xi2 = -h/2): von Mises stress
 * (RMShellPDE.von_Mises_stress(surface=...), rm_shell/rm_shell_pde.py:153-165) L2-projected onto DG1, nvc*nel values
 * (cell-major, the cell's vertices in connectivity order) -- replaces FEA.projectFieldOutput (fea/fea_dolfinx.py:205-206,
 * csdl_alpha_opt/output_operation.py:116-123). */
int femo_field_output(femo_ctx* ctx, const char* name, double* out, int64_t n);
/* Derivatives of the field outputs -- new: the reference's OutputFieldOperation declares them but defines no
 * compute_derivatives (csdl_alpha_opt/output_operation.py:72-128).  name = "stress" | "stress_mid" | "stress_bot";
 * wrt / arg = "disp_solid" (not for the totals), "thickness", "E", "nu", "uhat", "F_solid", "density" (the last two give
 * zeros).  Per cell the field is c_e = M_e^-1 b_e with a mass matrix M_e of the reference geometry, so only the von Mises
 * stress vm_q at the quadrature points is differentiated.  Zero-stress convention: a point with vm_q = 0 (w = 0, say)
 * contributes zero -- a subgradient, as for "pnorm_stress"; every derivative is finite there.  Sums over the cells run in
 * a fixed order without atomics: two identical calls return the same bits.
 * femo_field_output_vjp: nbar cotangents cbar (nbar x nvc*nel, cell-major like femo_field_output) -> out (nbar x n,
 *   n = the argument's length, femo_ndof for "disp_solid"): out_k = (d field / d wrt)^T cbar_k.
 * femo_field_output_jacobian_nnz / femo_field_output_jacobian: the partial Jacobian d field / d wrt as CSR with nvc*nel
 *   rows (row nvc*e + i: vertex i of cell e) and a fixed number of entries per row -- ld = 3 npc + 3 nvc for "disp_solid",
 *   nvc for nodal (1 for per-cell) "thickness" / "E" / "nu", 3 nvc for "uhat", 0 for "F_solid" / "density"; rowptr has
 *   nvc*nel + 1 entries, the columns of a row follow the cell's local order (not sorted).  nnz must be the count
 *   femo_field_output_jacobian_nnz returns.
 * femo_field_total_gradients: total derivatives of g_k = cbar_k . field through the solved state, for nbar cotangents:
 *   lambda_k = K^-1 (d field / d w)^T cbar_k (one grouped multi-right-hand-side solve, strong-BC rows masked, as in
 *   femo_total_gradients), out_k = (d field / d arg)^T cbar_k - (dR / d arg)^T lambda_k (nbar x n); iters, relres:
 *   nbar entries or NULL.
 * name = "ply_failure_field" (laminate mode with a table; csrc/ply_field_rev.h): a cotangent has nel * npt entries, cell-major like
 * femo_ply_failure_field; the maximiser convention is stated at femo_set_ply_table above and is the forward mode's.
 *   femo_field_output_vjp: wrt "disp_solid" and "ply_table" (16 npt nel, cell-major); exact zeros for "laminate", "thickness", "E",
 *     "nu", "density", "F_solid"; under an active layup "ply_thickness" / "ply_angle", the table cotangent pulled back through the
 *     layup on the device.  Row k of the result has the bits of the single call on cbar_k.
 *   femo_field_output_jacobian(_nnz): nel * npt rows (row npt*e + p), ld entries per row for "disp_solid" (columns in the cell's
 *     local order), 16 for "ply_table" (columns 16 (npt*e + p) + k), 0 for the six arguments above; the layup names are refused.
 *   femo_field_total_gradients: arg "laminate" and "F_solid" (no explicit partial), "ply_table", "thickness", "E", "nu", "density"
 *     (R does not depend on them in laminate mode: no solve runs, iters and relres come back 0), and "ply_thickness" / "ply_angle":
 *     -(dR / d laminate)^T lambda_k and (d field / d table)^T cbar_k through one pull-back of the layup.  k local failure constraints
 *     cost ceil(k / 4) grouped adjoint solves.
 *   Refused (nothing is written): "uhat" (the shape derivative of this output is not provided), a missing table (the message names
 *   femo_set_ply_table), a wrong n.  No float atomics, fixed summation orders: two identical calls return the same bits. */
int femo_field_output_vjp(femo_ctx* ctx, const char* name, const char* wrt, const double* cbar, int64_t nbar, double* out, int64_t n);
int femo_field_output_jacobian_nnz(femo_ctx* ctx, const char* name, const char* wrt, int64_t* nnz);
int femo_field_output_jacobian(femo_ctx* ctx, const char* name, const char* wrt, int64_t* rowptr, int32_t* colidx, double* vals,
                               int64_t nnz);
int femo_field_total_gradients(femo_ctx* ctx, const char* name, int32_t nbar, const double* cbar, const char* arg, double* out,
                               int64_t n, int32_t* iters, double* relres);
/* Forward mode of the field outputs, matrix-free: out[k] = (d field / d wrt) V[k] at the stored state and fields, k < ndir.
 * V: ndir x n, row-major, n the length of ONE direction (femo_ndof for "disp_solid", else femo_field_size(wrt)); out: ndir x nout,
 * nout the field's length (checked).
 *   name "stress" | "stress_mid" | "stress_bot" (layout of femo_field_output): wrt as for femo_field_output_vjp; "F_solid" and
 *     "density" give exact zeros, "stress_mid" with "thickness" too, and in laminate mode "laminate" and "ply_table" (these fields
 *     keep the single-layer recovery).  The zero-stress convention is that of the reverse products.
 *   name "ply_failure_field" (laminate mode with a table; nout = nel * npt, layout of femo_ply_failure_field; the maximiser
 *     convention is stated at femo_set_ply_table above): wrt "disp_solid" or "ply_table"; "laminate", "thickness", "E", "nu",
 *     "density" and "F_solid" give exact zeros; "uhat" is refused like the aggregate's shape derivative.
 * Every cell owns its entries of the output: plain stores, no float atomics, two identical calls return the same bits, and ndir
 * directions in one call give the bits of ndir single calls.  Refused (nothing is written): an unknown field output, an unknown
 * argument, a wrong n or nout, no ply table (the message names femo_set_ply_table), ndir < 1.  The state, the fields and the
 * factor are never written.
 * femo_field_total_jvp: the forward chain for fields.  dW[k] = -K^-1 (dR/d arg) V[k] by the code path of femo_total_jvp (grouping,
 * strong-row masking, option "strict" with status 4 and the refusals are the same; arg as there, "F_solid" and "laminate"
 * included), then for every named field d field[k] = (d field / d w) dW[k] + (d field / d arg) V[k]; the tangent states never
 * leave the device, and one tangent solve per direction serves every named field.  out holds the fields one after another in the
 * order of names, each an ndir x size_i block; nout = the sum of the sizes (checked).  Names may mix stress fields and the ply
 * failure field; "uhat" together with "ply_failure_field" is refused before any solve.  dW (ndir x ndof), iters and relres (ndir
 * entries) may be NULL. */
int femo_field_output_jvp(femo_ctx* ctx, const char* name, const char* wrt, int32_t ndir, const double* V, int64_t n, double* out,
                          int64_t nout);
int femo_field_total_jvp(femo_ctx* ctx, int32_t nnames, const char* const* names, const char* arg, int32_t ndir, const double* V,
                         int64_t n, double* out, int64_t nout, double* dW, int32_t* iters, double* relres);
/* Scalar outputs for the stored state and fields: "compliance", "mass", "elastic_energy", "pnorm_stress", "volume",
 * "regularization" (the thickness term of the compliance, rm_shell_pde.py:64-83), and over the selected sub-domain
 * (femo_select_subdomain; the whole mesh if none) "tip_disp" = 0.5 int u.u J, "area" = int J (rm_shell_pde.py:95-105) and
 * "sum_stress_x|y|z|xy|xz|yz" = int sigma_ij J dx of the top-surface in-plane stress (sum_stress_subdomain, :130-150), and in laminate
 * mode with a ply table "ply_failure" (femo_set_ply_table), and over the selected nodes "max_disp", "max_disp1", "max_disp2", "max_disp3"
 * (femo_set_disp_aggregate) --
 * replaces assemble_scalar(form(c)) (csdl_alpha_opt/output_operation.py:51-56; forms at
 * rm_shell/rm_shell_pde.py:64-110). */
int femo_functional(femo_ctx* ctx, const char* name, double* value);
/* Gradient vector of a scalar output with respect to "disp_solid", "thickness", "density", "E", "nu",
 * "F_solid" or "uhat" (zeros where the form does not depend on the argument; "uhat" = shape sensitivity
 * through F = I + grad(uhat), kinematics.py:12-44) -- replaces assemble(derivative(form, arg), dim=1)
 * (csdl_alpha_opt/output_operation.py:58-69). n must equal the argument's length. */
int femo_dfunctional(femo_ctx* ctx, const char* name, const char* wrt, double* out, int64_t n);
/* out = (dR/d arg)^T lambda at the stored state, arg in "thickness","E","nu","F_solid","uhat" --
 * replaces assembleMatrix(dR/d arg) + computeMatVecProductBwd
 * (csdl_alpha_opt/state_operation.py:174-184,283-286; fea/utils_dolfinx.py:294-306). */
int femo_dRdarg_T(femo_ctx* ctx, const char* arg, const double* lambda, double* out, int64_t n);
/* Forward mode of the same operator: out[k] = (dR/d arg) V[k], k < ndir; V: ndir x femo_field_size(arg), out: ndir x ndof, row-major;
 * n = femo_field_size(arg), the length of ONE direction -- replaces assembleMatrix(dR/d arg) + computeMatVecProductFwd
 * (csdl_alpha_opt/state_operation.py:159-171; fea/utils_dolfinx.py:275-283).  arg as for femo_dRdarg_T ("laminate" in laminate mode,
 * where "thickness", "E" and "nu" give exact zeros, as their transposes do).  R is the residual femo_residual returns: rows of
 * strong Dirichlet DOFs are zero (R = w - g there), and the state enters with those rows zeroed.  Element results are summed in a
 * fixed order without float atomics: two identical calls return the same bits. */
int femo_residual_jvp(femo_ctx* ctx, const char* arg, int32_t ndir, const double* V, int64_t n, double* out);
/* The forward chain on the device: dW[k] = -K^-1 (dR/d arg) V[k] (grouped through femo_solve_linear_multi: four tangents share a
 * pair of sweeps), dJ[i*ndir + k] = dJ_i/dw . dW[k] + dJ_i/d arg . V[k] for the named functionals (subdomains as in
 * femo_total_gradients).  dW (ndir x ndof) may be NULL (tangent states not wanted), nfun may be 0; iters, relres: ndir entries or
 * NULL.  One tangent solve per direction gives the derivative of every output -- what CSDL's forward mode assembles from
 * StateOperation.compute_jacvec_product('fwd') and apply_inverse_jacobian('fwd') (csdl_alpha_opt/state_operation.py:159-171, 188-220).
 * Refusals and status 4 (option "strict") as in femo_total_gradients; the state, the factor and the fields are never written. */
int femo_total_jvp(femo_ctx* ctx, const char* arg, int32_t ndir, const double* V, int64_t n, int32_t nfun, const char* const* functionals,
                   const int32_t* subdomains, double* dW, double* dJ, int32_t* iters, double* relres);

/* The whole adjoint chain on the device, no host round trips:
 *   lambda = K^-1 dJ/dw ;  out = dJ/d arg - (dR/d arg)^T lambda      (total derivative)
 * for J = "compliance" | "elastic_energy" | "mass" and arg = "thickness" | "E" | "nu" | "F_solid".
 * This is what CSDL's compute_totals assembles from OutputOperation.compute_derivatives,
 * StateOperation.apply_inverse_jacobian('rev') and compute_jacvec_product('rev')
 * (SURVEY.md section 3.3). */
int femo_total_gradient(femo_ctx* ctx, const char* functional, const char* arg, double* out, int64_t n,
                        int32_t* iters, double* relres);
/* The same for SEVERAL functionals of the state and one argument: the reference registers compliance, elastic_energy, pnorm_stress and
 * one pnorm_stress_<tag> per sub-domain on `disp_solid` (rm_shell_model.py:221-253) and the simulator solves one adjoint per output
 * (state_operation.py:188-220); here the adjoint right-hand sides dJ_i/dw are formed together and solved by femo_solve_linear_multi's
 * grouped sweeps.  subdomains[i]: the tagged sub-domain functional i is restricted to (femo_set_cell_tags; -1, or subdomains == NULL:
 * the whole mesh).  out: nfun x n, row i = d J_i / d arg; iters, relres: nfun entries or NULL. */
int femo_total_gradients(femo_ctx* ctx, int32_t nfun, const char* const* functionals, const int32_t* subdomains, const char* arg, double* out,
                         int64_t n, int32_t* iters, double* relres);

/* Timing of the most recent solve, measured with HIP events on the context's stream (ms):
 * [0] setup (diagonal / preconditioner), [1] Krylov loop (with option "stale_factor": a factorisation inside the loop included),
 * [2] total, [3] the multifrontal factor that preconditioned the solve: 0 the current operator's, 1 one kept from an earlier
 * design (option "stale_factor"), 2 a kept one that was refreshed inside the solve; [4] number of element-operator launches. */
int femo_last_timing(const femo_ctx* ctx, double* out5);

/* Average duration (ms) of `reps` back-to-back launches of one kernel, timed with HIP events on
 * the context's stream: "apply" (matrix-free element operator), "pcg_update", "pcg_direction", "diag"; with a ply table
 * "ply_value" (the aggregate's value pass), "ply_dw" (its state gradient as femo_dfunctional enqueues it: value pass, gradient
 * kernel, gather), "ply_field_vjp" (the field's reverse product with respect to the state: kernel and gather) and
 * "ply_field_vjp_table" (with respect to the table), the last two for a cotangent of ones. */
int femo_bench_kernel(femo_ctx* ctx, const char* name, int32_t reps, double* avg_ms);

/* ---- Building blocks of the element-partitioned multi-GPU driver (femo_alpha_amd/parallel.py).  The
 * reference has no multi-rank path (its meshes live on MPI.COMM_SELF, fea/utils_dolfinx.py:41); these
 * calls expose the local pieces between which the driver places its collectives.
 * Vector ids: 0 state, 1 adjoint, 2 r, 3 z, 4 p, 5 Ap, 6 b. */
void* femo_vec_ptr(femo_ctx* ctx, int32_t id);                 /* device pointer, femo_ndof doubles */
int femo_sync(femo_ctx* ctx);                                  /* wait for the context's stream */
void* femo_stream_ptr(femo_ctx* ctx);                          /* the context's hipStream_t: the multi-GPU driver makes it torch's
                                                                  current stream, so that its tensor ops and collectives are
                                                                  ordered with the library's launches without device-wide syncs */
int femo_op_apply_vec(femo_ctx* ctx, int32_t src, int32_t dst);   /* dst = K_local src (no Dirichlet mask) */
int femo_load_vec(femo_ctx* ctx, int32_t dst);                 /* dst = local load vector */
int femo_factorize_range(femo_ctx* ctx, int32_t l0, int32_t l1, int assemble);   /* tree levels [l0, l1) */
int femo_frontal_sweep(femo_ctx* ctx, int32_t vec, int32_t l0, int32_t l1, int backward);
int femo_front_schur_get(femo_ctx* ctx, int32_t front, void* dst_dev, int64_t capacity_doubles);
int femo_front_block_set(femo_ctx* ctx, int32_t front, const void* src_dev);
int femo_functionals_partial(femo_ctx* ctx, double* out3);     /* { int u.u J dx, regularisation, mass } */
int femo_dfunctional_vec(femo_ctx* ctx, const char* name, int32_t dst);
int femo_field_gradient_vec(femo_ctx* ctx, const char* functional, const char* arg, int32_t lam, double* out, int64_t n);

/* The partitioned PCG itself (the counterpart of the reference's KSP solve, fea/utils_dolfinx.py:501-531, on an element
 * partition the reference does not have).  The replicated separator entries ("top", local indices top_idx, the same global
 * order on every rank), the weights of the global dot product (1 / nranks on replicated entries) and the scatter map of the
 * gradient (sel: position of this rank's field entries in the global field) stay resident in the context.  Every call
 * below only ENQUEUES work on the context's stream; the caller issues the collective named in the comment on the same
 * stream (torch.distributed over RCCL) and is the only party that talks to other ranks.
 *   buffer 0 = ntop + 1 doubles: packed replicated entries + one scalar that rides along;   buffer 1 = the 8 device
 *   scalars, [1] = r.z. */
int femo_dist_setup(femo_ctx* ctx, int32_t ntop, const int32_t* top_idx, int32_t nranks, int32_t n_local_levels,
                    int32_t nsel, const int32_t* sel);
void* femo_dist_ptr(femo_ctx* ctx, int32_t which);
int femo_dist_pack(femo_ctx* ctx, int32_t vec);                /* buffer 0 = vec[top]            -> all-reduce(buffer 0[0..ntop)) */
int femo_dist_unpack(femo_ctx* ctx, int32_t vec);              /* vec[top] = buffer 0 */
int femo_dist_pcg_start(femo_ctx* ctx, int32_t b, int32_t x);  /* x = 0, r = b, share of b.b */
int femo_dist_precond_fwd(femo_ctx* ctx);                      /* z = r, local forward sweep      -> all-reduce(buffer 0[0..ntop]) */
int femo_dist_read(femo_ctx* ctx, double* out2);               /* host: { r.r, previous p.Ap } (the one synchronisation per iteration) */
int femo_dist_precond_rest(femo_ctx* ctx);                     /* top sweeps, local backward sweep -> all-reduce(buffer 1[1]) */
int femo_dist_direction_apply(femo_ctx* ctx, int first);       /* p, Ap = A_local p               -> all-reduce(buffer 0[0..ntop]) */
int femo_dist_update(femo_ctx* ctx, int32_t x);                /* x += alpha p, r -= alpha Ap */
/* gglob[sel] = d functional / d arg - (dR/d arg)^T lambda(vector id) over this rank's cells; gglob: device, zeroed by the
 * caller, summed over the ranks by the caller                                                      -> all-reduce(gglob) */
int femo_dist_gradient(femo_ctx* ctx, const char* functional, const char* arg, int32_t lam, void* gglob_dev, int64_t nglob);
/* packed lower triangle (column by column) of a front's Schur complement, and back into a pivot-free stand-in front: what
 * the all-gather of the subtree roots carries.  Asynchronous on the context's stream. */
int femo_front_schur_pack(femo_ctx* ctx, int32_t front, void* dst_dev, int64_t capacity_doubles);
int femo_front_block_unpack(femo_ctx* ctx, int32_t front, const void* src_dev);
/* per-class times / launches / flops / bytes of the factorisation launches since the last assembly while option
 * "profile" is on (same layout as femo_factorize_profile): the partitioned driver factorises in two ranges */
int femo_factorize_profile_get(femo_ctx* ctx, double* out32);

/* ---- Transient march (BASELINE config 5) -- replaces PlateSim.solve_dynamic_problem (dynamic_rm_shell/plate_sim.py:281-361:
 * per step update_f + solveNonlinear_mod + the velocity update of :243-244,333) and the backward sweep of the dynamic
 * StateOperation (state_operation_dynamic.py:406-427, 619-691).  Displacement history, pressure history, velocity and the
 * adjoint history stay resident in HBM; one call marches all steps.  Time discretisation of plate_sim.py:131-140:
 *   (a M + K/2) w_i = F_i + M (a w_{i-1} + b wdot_{i-1}) - K/2 w_{i-1},   a = 2/dt^2, b = 2/dt,   force at the new level.
 * Histories cross the boundary level-major: (time_levels x femo_ndof) row-major. */
int femo_newmark_setup(femo_ctx* ctx, int32_t time_levels, double dt);          /* allocates; selects the operator K/2 + a M */
int femo_newmark_set_forces(femo_ctx* ctx, const double* f_history, int32_t levels_given);   /* (levels x F_solid length) */
int femo_newmark_set_constant_load(femo_ctx* ctx, const double* F);             /* ndof load vector added to every step, or NULL */
int femo_newmark_march(femo_ctx* ctx, int32_t nsteps, int reassemble_every_step, int32_t* iters, double* relres);
int femo_newmark_get_history(femo_ctx* ctx, int32_t which, double* out);        /* which: 0 displacements, 2 adjoint */
int femo_newmark_set_history(femo_ctx* ctx, int32_t which, const double* H);   /* which: 0 displacements, 2 adjoint */
int femo_newmark_adjoint(femo_ctx* ctx, const double* G, int32_t levels);       /* (dR/dy)^T Lambda = G, O(T) recursion */
int femo_newmark_residual_T(femo_ctx* ctx, int32_t levels, double* g_thickness, double* dF);
/* The O(T) recursion of femo_newmark_adjoint run from the seed already in the adjoint seed buffer (left there by
 * femo_newmark_stress_history_grad(.., seed_adjoint = 1)), with no host copy.  The same seed gives the same bits as
 * femo_newmark_adjoint. */
int femo_newmark_adjoint_seeded(femo_ctx* ctx, int32_t levels);
/* Space-time p-norm stress aggregate of the transient path: S = sum_{i < levels} P_i, P_i = 1/alpha [int (m vm_top(w_i))^rho dx_4
 * + regc int t^rho dx_4], i.e. the sum over the time levels of the reference's PlateSim.pnorm_stress(level=i)
 * (dynamic_rm_shell/plate_sim.py:427-449) -- the stress constraint ex_gust_response_opt.py:320,329,724 and
 * ex_lpc_gust_response_opt.py:49,55,445 leave commented out.  m, rho: femo_set_stress_params; alpha: femo_set_stress_alpha(sel = -1)
 * (default the area of the degree-4 measure); regc: option "stress_regularization".  H: the history, (levels x ndof) level-major, or
 * NULL for the one of the last march, read in place.  A given H goes to a buffer of its own: the resident displacement history is
 * never written.  per_level (levels entries) and total may be NULL.  A P_i or S that is not finite is an error naming m and rho.
 * femo_newmark_stress_history_grad: g_thickness = dS/dt (thickness length; may be NULL), G = dS/dW (levels x ndof, level-major; may be
 * NULL); seed_adjoint != 0 leaves dS/dW in the adjoint seed buffer for femo_newmark_adjoint_seeded.  No float atomics: the results
 * repeat bit for bit. */
int femo_newmark_stress_history(femo_ctx* ctx, int32_t levels, const double* H, double* per_level, double* total);
int femo_newmark_stress_history_grad(femo_ctx* ctx, int32_t levels, const double* H, double* g_thickness, double* G, int seed_adjoint);
/* Max-displacement aggregate of the transient path: the lpc example's max_disp = csdl.maximum(csdl.absolute(s*disp_history),
 * rho=rho_max)/s (ex_lpc_gust_response_opt.py:457-459, 770-772; rho_max = 300 at :77, s = 1/max(tip_disp_history)), a KS aggregate
 * over every entry of the space-time history.  Our contract (csdl_alpha's maximum / absolute are not checked against it): for
 * rho > 0 and a finite s != 0, x_k = |s| |w_k| over the selected entries k,
 *     M = ( x_max + 1/rho log sum_k exp(rho (x_k - x_max)) ) / s,      dM/dw_k = sign(s) sign(w_k) exp(rho (x_k - s M))
 * (0 where w_k = 0 and on entries not selected; every exponent <= 0).  components: 0 every entry (rotations included, as the example
 * aggregates), 1 the first ndof_u entries of every level (the mid-surface displacement).  H: (levels x ndof) level-major, or NULL for
 * the history of the last march, read in place; a given H goes to the buffer of femo_newmark_stress_history, never into the resident
 * history.  per_level (levels entries: M_l over level l alone) and total may be NULL.  rho <= 0, s zero or not finite, and a
 * non-finite history entry (the level is named) are errors.  femo_newmark_disp_aggregate_grad: total = M (the same bits as
 * femo_newmark_disp_aggregate), G = dM/dW (levels x ndof, level-major; may be NULL); seed_adjoint != 0 leaves dM/dW in the adjoint
 * seed buffer for femo_newmark_adjoint_seeded.  No float atomics: the results repeat bit for bit. */
int femo_newmark_disp_aggregate(femo_ctx* ctx, int32_t levels, const double* H, int32_t components, double rho, double scaler,
                                double* per_level, double* total);
int femo_newmark_disp_aggregate_grad(femo_ctx* ctx, int32_t levels, const double* H, int32_t components, double rho, double scaler,
                                     double* total, double* G, int seed_adjoint);
/* Forward mode (state_operation_dynamic.py:228-329: compute_jacvec_product fwd; :534-605: apply_inverse_jacobian fwd, the
 * "tangent linear model").  Results land in the adjoint-history buffer (femo_newmark_get_history(ctx, 2, ..)). */
int femo_newmark_jvp(femo_ctx* ctx, int32_t levels, const double* dY, const double* dthickness, const double* dF);
int femo_newmark_tangent(femo_ctx* ctx, const double* dR, int32_t levels);
/* Device addresses of the resident buffers: 0 displacement history, 1 velocity of the last level the march reached, 2 adjoint /
 * tangent history.  Lifetime: until the next femo_newmark_setup on this context (which re-allocates them) or femo_destroy; a
 * caller that wraps them (the zero-copy torch views of PlateSim) must drop its views before either. */
void* femo_newmark_ptr(femo_ctx* ctx, int32_t which);

/* Raw device pointer of a named buffer ("state","thickness","E","nu","density","F_solid","uhat")
 * for zero-copy wrapping by the caller (e.g. torch.from_dlpack-free ctypes views). */
void* femo_device_ptr(femo_ctx* ctx, const char* name);

#ifdef __cplusplus
}
#endif
#endif /* FEMO_HIP_H */
