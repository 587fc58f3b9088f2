"""CPU reference of the load-proportional ply strength index (include/femo_hip.h, "ply_strength_index" and
"ply_strength_index_field"), numpy only, written from the contract on top of tests/ply_failure_ref.py:

    b = F1 s1 + F2 s2,   a = F11 s1^2 + F22 s2^2 + F66 t12^2 + 2 F12 s1 s2,   D = sqrt(max(b^2 + 4 a, 0))
    r = (b + D) / 2 (b >= 0),   r = 2 a / (D - b) (b < 0),   r = 0 where D = 0;   dr = (r db + da) / D, 0 where D = 0
    K = 1/rho log( 1/(alpha npt) sum_e sum_q w_q det_q J_q sum_p exp(rho r_eqp) )

``failure_index`` returns r, so ``value``, ``field`` and ``bounds`` of the parent are those of the new outputs.  Every routine carries
complex arithmetic (branches and guards decide on real parts), so the derivatives can be checked against complex steps of the value."""
import numpy as np

from ply_failure_ref import PlyFailureOracle


class PlyStrengthOracle(PlyFailureOracle):
    @staticmethod
    def ab_of(table, s):
        """a, b (nel, nq, npt), sigma and x = eps - z kappa (nel, nq, npt, 3)."""
        _, sig, x = PlyFailureOracle.fi_of(table, s)
        F = table[:, None, :, 10:16]
        s1, s2, t = sig[..., 0], sig[..., 1], sig[..., 2]
        b = F[..., 0] * s1 + F[..., 1] * s2
        a = F[..., 2] * s1 * s1 + F[..., 3] * s2 * s2 + F[..., 4] * t * t + 2 * F[..., 5] * s1 * s2
        return a, b, sig, x

    @staticmethod
    def r_of(table, s):
        """r, 1 / D (0 where D = 0), sigma, x."""
        a, b, sig, x = PlyStrengthOracle.ab_of(table, s)
        t = b * b + 4 * a
        D = np.sqrt(np.where(t.real < 0, 0.0, t))
        zero = D.real == 0
        Ds = np.where(zero, 1.0, D)
        neg = b.real < 0
        den = np.where(neg, Ds - b, 1.0)
        r = np.where(neg, 2 * a / den, 0.5 * (b + D))
        r = np.where(zero, 0.0, r)
        iD = np.where(zero, 0.0, 1.0 / Ds)
        return r, iD, sig, x

    def failure_index(self, w, table=None):
        s, wj, wd, _ = self.strains(w)
        return self.r_of(self.ply if table is None else table, s)[0], wj, wd

    def _dr(self, table, sig, r, iD, c):
        """c dr / dsigma (..., 3) and c dr / d(F1, F2, F11, F22, F66, F12) (..., 6) on the (nel, nq, npt) or (nel, npt) grid of c."""
        F = table[:, None, :, 10:16] if c.ndim == 3 else table[:, :, 10:16]
        s1, s2, t = sig[..., 0], sig[..., 1], sig[..., 2]
        ci = c * iD
        sb = np.stack([ci * (r * F[..., 0] + 2 * F[..., 2] * s1 + 2 * F[..., 5] * s2),
                       ci * (r * F[..., 1] + 2 * F[..., 3] * s2 + 2 * F[..., 5] * s1), ci * 2 * F[..., 4] * t], axis=-1)
        fb = np.stack([ci * r * s1, ci * r * s2, ci * s1 * s1, ci * s2 * s2, ci * t * t, 2 * ci * s1 * s2], axis=-1)
        return sb, fb

    def gradients(self, w, rho, cells=None):
        """(dK/dw (ndof), dK/dtable (nel, npt, 16))."""
        s, wj, wd, B = self.strains(w)
        r, iD, sig, x = self.r_of(self.ply, s)
        sel = self._cells(cells)
        u = rho * r
        shift = np.max(u[sel])
        c = wj[:, :, None] * np.exp(u - shift) * sel[:, None, None]
        c = c / c.sum()                                              # dK / dr_eqp
        sb, fb = self._dr(self.ply, sig, r, iD, c)
        G = self.ply[:, :, 0:9].reshape(self.mesh.nel, -1, 3, 3)
        z = self.ply[:, :, 9]
        xb = np.einsum("epij,eqpi->eqpj", G, sb)
        sbar = np.concatenate([xb.sum(axis=2), -(z[:, None, :, None] * xb).sum(axis=2)], axis=-1)
        ge = np.einsum("eqik,eqi->ek", B, sbar)
        gw = np.zeros(self.mesh.ndof)
        np.add.at(gw, self.dofs.ravel(), ge.ravel())
        gt = np.zeros((self.mesh.nel, self.npt, 16))
        gt[:, :, 0:9] = np.einsum("eqpi,eqpj->epij", sb, x).reshape(self.mesh.nel, self.npt, 9)
        gt[:, :, 9] = -np.einsum("eqpj,eqj->ep", xb, s[:, :, 3:6])
        gt[:, :, 10:16] = fb.sum(axis=1)
        return gw, gt

    def field_vjp(self, w, cbar, table=None):
        """((d field / d w)^T cbar (ndof), (d field / d table)^T cbar (nel, npt, 16)) for cbar (nel, npt): the derivative of r at the
        first quadrature point that attains the maximum."""
        table = self.ply if table is None else table
        nel, npt = table.shape[0], table.shape[1]
        s, _, _, B = self.strains(w)
        r, iD, sig, x = self.r_of(table, s)
        qmax = r.argmax(axis=1)
        e_idx, p_idx = np.arange(nel)[:, None], np.arange(npt)[None, :]
        r, iD, sig, x = r[e_idx, qmax, p_idx], iD[e_idx, qmax, p_idx], sig[e_idx, qmax, p_idx], x[e_idx, qmax, p_idx]
        kap = s[e_idx, qmax][..., 3:6]
        Bq = B[e_idx, qmax]                                           # (nel, npt, 6, ldof)
        sb, fb = self._dr(table, sig, r, iD, np.asarray(cbar).reshape(nel, npt))
        G = table[:, :, 0:9].reshape(nel, npt, 3, 3)
        z = table[:, :, 9]
        xb = np.einsum("epij,epi->epj", G, sb)
        ge = (np.einsum("epj,epjk->ek", xb, Bq[:, :, 0:3]) - np.einsum("ep,epj,epjk->ek", z, xb, Bq[:, :, 3:6]))
        gw = np.zeros(self.mesh.ndof)
        np.add.at(gw, self.dofs.ravel(), ge.ravel())
        gt = np.zeros((nel, npt, 16))
        gt[..., 0:9] = np.einsum("epi,epj->epij", sb, x).reshape(nel, npt, 9)
        gt[..., 9] = -np.einsum("epj,epj->ep", xb, kap)
        gt[..., 10:16] = fb
        return gw, gt
