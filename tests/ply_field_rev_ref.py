"""numpy reference of the reverse mode of the ply failure field (include/femo_hip.h, femo_field_output_vjp / _jacobian with the
name "ply_failure_field"), written from the contract on top of tests/ply_failure_ref.py: an entry of the field is max_q FI_eqp, its
derivative the derivative of FI at the first quadrature point that attains the maximum (``fi.argmax(axis=1)``).  The two partial
Jacobians are built as sparse matrices from the B rows of ``o.strains``; products with them are the reference of both modes."""
import numpy as np
import scipy.sparse as sp


def ply_field_jacobians(o, w, table):
    """(J_w (nel npt, ndof), J_t (nel npt, 16 npt nel)) as CSR at state ``w`` and table ``table`` (nel, npt, 16); row e npt + p, the
    table columns cell-major like the table itself."""
    nel, npt = table.shape[0], table.shape[1]
    s, _, _, B = o.strains(w)                                                      # (nel, nq, 6), (nel, nq, 6, ldof)
    fi, sig, x = o.fi_of(table, s)
    qmax = fi.argmax(axis=1)                                                       # (nel, npt): the first maximiser in quadrature order
    e_idx = np.arange(nel)[:, None]
    p_idx = np.arange(npt)[None, :]
    sig = sig[e_idx, qmax, p_idx]                                                  # (nel, npt, 3) at the maximiser
    x = x[e_idx, qmax, p_idx]
    kap = s[e_idx, qmax][..., 3:6]                                                 # (nel, npt, 3)
    Bq = B[e_idx, qmax]                                                            # (nel, npt, 6, ldof)
    G = table[:, :, 0:9].reshape(nel, npt, 3, 3)
    z = table[:, :, 9]
    F = table[:, :, 10:16]
    s1, s2, t = sig[..., 0], sig[..., 1], sig[..., 2]
    sb = np.stack([F[..., 0] + 2 * F[..., 2] * s1 + 2 * F[..., 5] * s2, F[..., 1] + 2 * F[..., 3] * s2 + 2 * F[..., 5] * s1,
                   2 * F[..., 4] * t], axis=-1)                                   # dFI / dsigma (nel, npt, 3)
    xb = np.einsum("epij,epi->epj", G, sb)                                         # dFI / dx = G^T sbar
    rows_w = np.einsum("epj,epjk->epk", xb, Bq[:, :, 0:3]) - z[..., None] * np.einsum("epj,epjk->epk", xb, Bq[:, :, 3:6])
    ldof = rows_w.shape[-1]
    cols_w = np.broadcast_to(o.dofs[:, None, :], (nel, npt, ldof))
    Jw = sp.csr_matrix((rows_w.ravel(), cols_w.ravel(), np.arange(nel * npt + 1) * ldof), shape=(nel * npt, o.mesh.ndof))
    rows_t = np.empty((nel, npt, 16))
    rows_t[..., 0:9] = np.einsum("epi,epj->epij", sb, x).reshape(nel, npt, 9)
    rows_t[..., 9] = -np.einsum("epj,epj->ep", xb, kap)
    rows_t[..., 10] = s1
    rows_t[..., 11] = s2
    rows_t[..., 12] = s1 * s1
    rows_t[..., 13] = s2 * s2
    rows_t[..., 14] = t * t
    rows_t[..., 15] = 2 * s1 * s2
    Jt = sp.csr_matrix((rows_t.ravel(), np.arange(16 * npt * nel), np.arange(nel * npt + 1) * 16), shape=(nel * npt, 16 * npt * nel))
    return Jw, Jt
