"""numpy reference of the forward mode of the ply failure field (include/femo_hip.h, femo_field_output_jvp), written from the
contract on top of tests/ply_failure_ref.py: an entry of the field is max_q FI_eqp, its tangent the tangent of FI at the first
quadrature point that attains the maximum.  The strains are linear in the state, so ``o.strains(dw)`` are the tangent strains."""
import numpy as np


def fi_gap(fi):
    """(nel, npt): the largest FI over the quadrature points minus the second largest (fi: (nel, nq, npt))."""
    top = np.sort(fi, axis=1)
    return top[:, -1] - top[:, -2]


def ply_field_tangent(o, w, table, dw=None, dtable=None):
    """(tangent (nel, npt), gap (nel, npt), max |FI|) of the field at state ``w`` and table ``table`` (nel, npt, 16) along a state
    direction ``dw`` and / or a table direction ``dtable``."""
    nel = table.shape[0]
    s = o.strains(w)[0]
    fi, sig, x = o.fi_of(table, s)
    G = table[:, :, 0:9].reshape(nel, -1, 3, 3)
    z = table[:, :, 9]
    F = table[:, None, :, 10:16]
    s1, s2, t = sig[..., 0], sig[..., 1], sig[..., 2]
    sb = np.stack([F[..., 0] + 2 * F[..., 2] * s1 + 2 * F[..., 5] * s2, F[..., 1] + 2 * F[..., 3] * s2 + 2 * F[..., 5] * s1,
                   2 * F[..., 4] * t], axis=-1)                                   # dFI / dsigma (nel, nq, npt, 3)
    dfi = np.zeros_like(fi)
    if dw is not None:
        ds = o.strains(dw)[0]
        dx = ds[:, :, None, 0:3] - z[:, None, :, None] * ds[:, :, None, 3:6]
        dfi += np.einsum("eqpi,epij,eqpj->eqp", sb, G, dx)
    if dtable is not None:
        dt = np.asarray(dtable).reshape(table.shape)
        dG = dt[:, :, 0:9].reshape(nel, -1, 3, 3)
        dz = dt[:, :, 9]
        dF = dt[:, None, :, 10:16]
        dsig = np.einsum("epij,eqpj->eqpi", dG, x) - dz[:, None, :, None] * np.einsum("epij,eqj->eqpi", G, s[:, :, 3:6])
        dfi += np.einsum("eqpi,eqpi->eqp", sb, dsig)
        dfi += dF[..., 0] * s1 + dF[..., 1] * s2 + dF[..., 2] * s1 * s1 + dF[..., 3] * s2 * s2 + dF[..., 4] * t * t + 2 * dF[..., 5] * s1 * s2
    qmax = fi.argmax(axis=1)                                                      # the first maximiser in quadrature order
    tan = np.take_along_axis(dfi, qmax[:, None, :], axis=1)[:, 0, :]
    return tan, fi_gap(fi), np.abs(fi).max()
