"""CPU reference of the laminated composite law: ``ShellOracle`` with the constitutive blocks of ``MaterialModelComposite`` /
``ElasticModelShapeOpt`` (femo_alpha/rm_shell/linear_shell_fenicsx/linear_shell_model.py:159-190, 268-296) in place of the single-layer
law.  Only ``_C`` changes: the strains, measures, penalty, load and outputs are the oracle's own."""
import numpy as np

from oracle.rm_shell_oracle import ShellOracle


class LaminateOracle(ShellOracle):
    def set_laminate(self, clt):
        """(nel, 32) per cell: [A, B, D (3x3 row-major), A_s (2x2), c_drill]."""
        self.clt = np.asarray(clt, dtype=np.float64).reshape(self.mesh.nel, 32)

    @staticmethod
    def _sym(X):
        return 0.5 * (X + np.swapaxes(X, -1, -2))

    def _C(self, sl, g, deriv=None):
        """Hessian of 1/2 (eps.A eps + eps.B kappa + kappa.B eps + kappa.D kappa) + 1/2 gamma.A_s gamma + 1/2 c_drill/h_K^2 omega^2
        times the measures of the isotropic path: strain rule without J (A, B, D), strain rule with J (A_s), full rule with J (drilling)."""
        if deriv is not None:
            raise ValueError("laminate mode: the law has no thickness / E / nu dependence")
        L = self.clt[sl]
        A, B, D = (self._sym(L[:, 9 * k: 9 * k + 9].reshape(-1, 3, 3)) for k in range(3))
        As = self._sym(L[:, 27:31].reshape(-1, 2, 2))
        cd = L[:, 31]
        wdet = self.wts[None, :] * g["det"]
        wdetS = self.wts_strain[None, :] * g["det"]
        Ju = g["Ju"]
        hK2 = self.hK[sl] ** 2
        C = np.zeros(wdet.shape + (9, 9), dtype=self.acc)
        C[..., 0:3, 0:3] = A[:, None] * wdetS[..., None, None]
        C[..., 0:3, 3:6] = B[:, None] * wdetS[..., None, None]
        C[..., 3:6, 0:3] = B[:, None] * wdetS[..., None, None]
        C[..., 3:6, 3:6] = D[:, None] * wdetS[..., None, None]
        C[..., 6:8, 6:8] = As[:, None] * (Ju * wdetS)[..., None, None]
        C[..., 8, 8] = (cd / hK2)[:, None] * Ju * wdet
        return C

    def dRdlam_T(self, w, lam, absolute=False):
        """(nel, 32): lam^T (dK / d laminate_e[k]) w, with the law acting through the symmetric parts.
        ``absolute``: the same sums with every term replaced by its absolute value (oracle/rm_shell_oracle.py: _ABSOLUTE)."""
        a = np.abs if absolute else (lambda v: v)
        out = np.zeros((self.mesh.nel, 32), dtype=self.acc)
        d = self.dofs
        for sl in self._chunks():
            B, g = self._B(sl)
            B = a(B)
            sw = np.einsum("eqik,ek->eqi", B, a(w[d[sl]]))
            sl_ = np.einsum("eqik,ek->eqi", B, a(lam[d[sl]]))
            wdet = a(self.wts[None, :] * g["det"])
            wdetS = a(self.wts_strain[None, :] * g["det"])
            Ju = a(g["Ju"])

            def outer(a, b, wt):                      # sum_q wt 1/2 (a_i b_j + a_j b_i)
                o = np.einsum("eq,eqi,eqj->eij", wt, a, b)
                return 0.5 * (o + np.swapaxes(o, -1, -2))
            ew, kw, gw = sw[..., 0:3], sw[..., 3:6], sw[..., 6:8]
            el, kl, gl = sl_[..., 0:3], sl_[..., 3:6], sl_[..., 6:8]
            out[sl, 0:9] = outer(el, ew, wdetS).reshape(-1, 9)
            out[sl, 9:18] = (outer(el, kw, wdetS) + outer(kl, ew, wdetS)).reshape(-1, 9)
            out[sl, 18:27] = outer(kl, kw, wdetS).reshape(-1, 9)
            out[sl, 27:31] = outer(gl, gw, Ju * wdetS).reshape(-1, 4)
            out[sl, 31] = np.einsum("eq,eq,eq->e", Ju * wdet / (self.hK[sl] ** 2)[:, None], sl_[..., 8], sw[..., 8])
        return out
