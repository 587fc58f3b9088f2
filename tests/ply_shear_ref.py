"""CPU reference of the interlaminar shear outputs (include/femo_hip.h, femo_set_ply_shear_table), numpy only, written from the
contract:

    wj_eq = w_q det_eq J_eq,   a_e = sum_q wj_eq,   gbar_e = (1/a_e) sum_q wj_eq (ga0, ga1)_eq
    (t13, t23)_ep = Gs_ep gbar_e,   FI_ep = F55 t13^2 + F44 t23^2
    K = 1/rho log( 1/(alpha npt) sum_e a_e sum_p exp(rho FI_ep) )

on the degree-4 rule, with the strains (rows 6 and 7 of ``_B``), geometry and weights of the oracle.  Build it as
``PlyShearOracle(mesh, nquad=degree4_rule(mesh), ...)``.  Every routine carries complex arithmetic through the mean, Gs gbar and the
polynomial, so that the derivatives can be checked against complex steps of the value."""
import numpy as np

from laminate_ref import LaminateOracle


class PlyShearOracle(LaminateOracle):
    def set_ply_shear_table(self, table, npt):
        self.npt_s = int(npt)
        self.psh = np.asarray(table).reshape(self.mesh.nel, self.npt_s, 6)

    def _cells(self, cells):
        return np.ones(self.mesh.nel, bool) if cells is None else np.isin(np.arange(self.mesh.nel), np.asarray(cells))

    def shear(self, w):
        """(nel, nq, 2) pointwise (ga0, ga1), the weights w det J (nel, nq), w det (nel, nq) and the two B rows (nel, nq, 2, ldof)."""
        S, WJ, WD, BB = [], [], [], []
        for sl in self._chunks():
            B, g = self._B(sl)
            S.append(np.einsum("eqik,ek->eqi", B[:, :, 6:8], w[self.dofs[sl]]))
            WD.append(self.wts[None, :] * g["det"])
            WJ.append(WD[-1] * g["Ju"])
            BB.append(B[:, :, 6:8])
        return np.concatenate(S), np.concatenate(WJ), np.concatenate(WD), np.concatenate(BB)

    def mean_shear(self, w):
        """gbar (nel, 2), a (nel,), w det (nel, nq), and the mean B rows (nel, 2, ldof) = sum_q (wj / a) B_q."""
        s, wj, wd, B = self.shear(w)
        a = wj.sum(axis=1)
        return np.einsum("eq,eqi->ei", wj, s) / a[:, None], a, wd, np.einsum("eq,eqik->eik", wj, B) / a[:, None, None]

    @staticmethod
    def fi_of(table, gbar):
        """FI (nel, npt) and t = Gs gbar (nel, npt, 2) from table (nel, npt, 6), gbar (nel, 2)."""
        Gs = table[:, :, 0:4].reshape(table.shape[0], -1, 2, 2)
        t = np.einsum("epij,ej->epi", Gs, gbar)
        return table[:, :, 4] * t[..., 0] * t[..., 0] + table[:, :, 5] * t[..., 1] * t[..., 1], t

    def field(self, w, table=None):
        """(nel, npt)."""
        return self.fi_of(self.psh if table is None else table, self.mean_shear(w)[0])[0]

    def value(self, w, rho, alpha=None, cells=None, table=None, shift=None):
        """K; log-sum-exp written out with a real shift (``shift``: given, or the largest real part)."""
        gbar, a, wd, _ = self.mean_shear(w)
        fi = self.fi_of(self.psh if table is None else table, gbar)[0]
        sel = self._cells(cells)
        alpha = np.sum(wd[sel]) if alpha is None else alpha
        u = rho * fi[sel]
        shift = np.max(u.real) if shift is None else shift
        tot = np.sum(a[sel][:, None] * np.exp(u - shift))
        return (shift + np.log(tot / (alpha * self.npt_s))) / rho

    def field_vjp(self, w, cbar):
        """((d field / d w)^T cbar (ndof), (d field / d table)^T cbar (nel, npt, 6)) for a cotangent cbar (nel, npt)."""
        gbar, a, wd, Bm = self.mean_shear(w)
        fi, t = self.fi_of(self.psh, gbar)
        c = np.asarray(cbar).reshape(fi.shape)
        tb = np.stack([2 * c * self.psh[:, :, 4] * t[..., 0], 2 * c * self.psh[:, :, 5] * t[..., 1]], axis=-1)     # d / dt (nel, npt, 2)
        Gs = self.psh[:, :, 0:4].reshape(self.mesh.nel, -1, 2, 2)
        gb = np.einsum("epij,epi->ej", Gs, tb)                        # d / dgbar
        ge = np.einsum("eik,ei->ek", Bm, gb)
        gw = np.zeros(self.mesh.ndof)
        np.add.at(gw, self.dofs.ravel(), ge.ravel())
        gt = np.zeros((self.mesh.nel, self.npt_s, 6))
        gt[:, :, 0:4] = np.einsum("epi,ej->epij", tb, gbar).reshape(self.mesh.nel, self.npt_s, 4)
        gt[:, :, 4] = c * t[..., 0] ** 2
        gt[:, :, 5] = c * t[..., 1] ** 2
        return gw, gt

    def gradients(self, w, rho, cells=None):
        """(dK/dw (ndof), dK/dtable (nel, npt, 6)): the field's reverse product with c_ep = a_e exp(rho FI_ep - S)."""
        gbar, a, _, _ = self.mean_shear(w)
        fi = self.fi_of(self.psh, gbar)[0]
        sel = self._cells(cells)
        u = rho * fi
        c = a[:, None] * np.exp(u - np.max(u[sel])) * sel[:, None]
        return self.field_vjp(w, c / c.sum())

    def bounds(self, w, rho, alpha=None, cells=None):
        """(lower, upper) of K for uhat = 0: max FI + 1/rho log(min_e a_e / (alpha npt)) <= K <= max FI."""
        gbar, a, wd, _ = self.mean_shear(w)
        fi = self.fi_of(self.psh, gbar)[0]
        sel = self._cells(cells)
        alpha = np.sum(wd[sel]) if alpha is None else alpha
        mx = fi[sel].max()
        return mx + np.log(a[sel].min() / (alpha * self.npt_s)) / rho, mx
