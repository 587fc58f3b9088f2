"""CPU reference of the ply failure outputs (include/femo_hip.h, femo_set_ply_table), numpy only, written from the contract:

    sigma = G (eps - z kappa),   FI = F1 s1 + F2 s2 + F11 s1^2 + F22 s2^2 + F66 t12^2 + 2 F12 s1 s2
    K = 1/rho log( 1/(alpha npt) sum_e sum_q w_q det_q J_q sum_p exp(rho FI_eqp) )

on the degree-4 rule, with the strains, geometry and weights of the oracle (``_B``).  Build it as
``PlyFailureOracle(mesh, nquad=degree4_rule(mesh), ...)``.  Every routine carries complex arithmetic through G (eps - z kappa) and the
polynomial, so that the derivatives can be checked against complex steps of the value."""
import numpy as np

from laminate_ref import LaminateOracle


class PlyFailureOracle(LaminateOracle):
    def set_ply_table(self, table, npt):
        self.npt = int(npt)
        self.ply = np.asarray(table).reshape(self.mesh.nel, self.npt, 16)

    def _cells(self, cells):
        return np.ones(self.mesh.nel, bool) if cells is None else np.isin(np.arange(self.mesh.nel), np.asarray(cells))

    def strains(self, w):
        """(nel, nq, 6) Voigt (eps, kappa), the weights w det J (nel, nq), w det (nel, nq) and the B rows (nel, nq, 6, ldof)."""
        S, WJ, WD, BB = [], [], [], []
        for sl in self._chunks():
            B, g = self._B(sl)
            S.append(np.einsum("eqik,ek->eqi", B[:, :, :6], w[self.dofs[sl]]))
            WD.append(self.wts[None, :] * g["det"])
            WJ.append(WD[-1] * g["Ju"])
            BB.append(B[:, :, :6])
        return np.concatenate(S), np.concatenate(WJ), np.concatenate(WD), np.concatenate(BB)

    @staticmethod
    def fi_of(table, s):
        """FI (nel, nq, npt), sigma (nel, nq, npt, 3) and x = eps - z kappa (nel, nq, npt, 3) from table (nel, npt, 16), s (nel, nq, 6)."""
        G = table[:, :, 0:9].reshape(table.shape[0], -1, 3, 3)
        z = table[:, :, 9]
        x = s[:, :, None, 0:3] - z[:, None, :, None] * s[:, :, None, 3:6]
        sig = np.einsum("epij,eqpj->eqpi", G, x)
        F = table[:, None, :, 10:16]
        s1, s2, t = sig[..., 0], sig[..., 1], sig[..., 2]
        fi = F[..., 0] * s1 + F[..., 1] * s2 + F[..., 2] * s1 * s1 + F[..., 3] * s2 * s2 + F[..., 4] * t * t + 2 * F[..., 5] * s1 * s2
        return fi, sig, x

    def failure_index(self, w, table=None):
        s, wj, wd, _ = self.strains(w)
        return self.fi_of(self.ply if table is None else table, s)[0], wj, wd

    def field(self, w):
        """(nel, npt): max over the quadrature points."""
        return self.failure_index(w)[0].max(axis=1)

    def area(self, cells=None):
        sel = self._cells(cells)
        return sum(np.sum((self.wts[None, :] * self._B(sl)[1]["det"])[sel[sl]]) for sl in self._chunks())

    def value(self, w, rho, alpha=None, cells=None, table=None, shift=None):
        """K; log-sum-exp written out with a real shift (``shift``: given, or the largest real part)."""
        fi, wj, wd = self.failure_index(w, table)
        sel = self._cells(cells)
        alpha = np.sum(wd[sel]) if alpha is None else alpha
        u = rho * fi[sel]
        shift = np.max(u.real) if shift is None else shift
        tot = np.sum(wj[sel][:, :, None] * np.exp(u - shift))
        return (shift + np.log(tot / (alpha * self.npt))) / rho

    def gradients(self, w, rho, cells=None):
        """(dK/dw (ndof), dK/dtable (nel, npt, 16))."""
        s, wj, wd, B = self.strains(w)
        fi, sig, x = self.fi_of(self.ply, s)
        sel = self._cells(cells)
        u = rho * fi
        shift = np.max(u[sel])
        c = wj[:, :, None] * np.exp(u - shift) * sel[:, None, None]
        c = c / c.sum()                                              # dK / dFI_eqp
        F = self.ply[:, None, :, 10:16]
        s1, s2, t = sig[..., 0], sig[..., 1], sig[..., 2]
        sb = np.stack([c * (F[..., 0] + 2 * F[..., 2] * s1 + 2 * F[..., 5] * s2), c * (F[..., 1] + 2 * F[..., 3] * s2 + 2 * F[..., 5] * s1),
                       c * 2 * F[..., 4] * t], axis=-1)              # dK / dsigma (nel, nq, npt, 3)
        G = self.ply[:, :, 0:9].reshape(self.mesh.nel, -1, 3, 3)
        z = self.ply[:, :, 9]
        xb = np.einsum("epij,eqpi->eqpj", G, sb)                      # dK / dx
        sbar = np.concatenate([xb.sum(axis=2), -(z[:, None, :, None] * xb).sum(axis=2)], axis=-1)     # (nel, nq, 6)
        ge = np.einsum("eqik,eqi->ek", B, sbar)
        gw = np.zeros(self.mesh.ndof)
        np.add.at(gw, self.dofs.ravel(), ge.ravel())
        gt = np.zeros((self.mesh.nel, self.npt, 16))
        gt[:, :, 0:9] = np.einsum("eqpi,eqpj->epij", sb, x).reshape(self.mesh.nel, self.npt, 9)
        gt[:, :, 9] = -np.einsum("eqpj,eqj->ep", xb, s[:, :, 3:6])
        gt[:, :, 10] = (c * s1).sum(axis=1)
        gt[:, :, 11] = (c * s2).sum(axis=1)
        gt[:, :, 12] = (c * s1 * s1).sum(axis=1)
        gt[:, :, 13] = (c * s2 * s2).sum(axis=1)
        gt[:, :, 14] = (c * t * t).sum(axis=1)
        gt[:, :, 15] = (2 * c * s1 * s2).sum(axis=1)
        return gw, gt

    def bounds(self, w, rho, alpha=None, cells=None):
        """(lower, upper) of K for uhat = 0: max FI + 1/rho log(min_eq(w det) / (alpha npt)) <= K <= max FI."""
        fi, wj, wd = self.failure_index(w)
        sel = self._cells(cells)
        alpha = np.sum(wd[sel]) if alpha is None else alpha
        mx = fi[sel].max()
        return mx + np.log(wd[sel].min() / (alpha * self.npt)) / rho, mx
