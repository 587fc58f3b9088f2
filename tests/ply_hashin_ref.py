"""CPU reference of the Hashin fibre and matrix failure outputs (include/femo_hip.h, "ply_hashin_fibre", "ply_hashin_matrix",
femo_ply_hashin_field and the two field names), numpy only, written from the contract on top of tests/ply_failure_ref.py:

    sigma = (s1, s2, t12) = G (eps - z kappa)                       G, z: entries 0..9 of the ply table
    fibre   FI_f = (s1/Xt)^2  (s1 >= 0),   (s1/Xc)^2  (s1 < 0)
    matrix  FI_m = (s2/Yt)^2 + (t12/SL)^2  (s2 >= 0),   (s2/(2 ST))^2 + c1 s2 + (t12/SL)^2  (s2 < 0),   c1 = ((Yc/(2 ST))^2 - 1)/Yc
    K = 1/rho log( 1/(alpha npt) sum_e sum_q w_q det_q J_q sum_p exp(rho FI_eqp) )

with strengths [Xt, Xc, Yt, Yc, SL, ST] per (cell, recovery point).  ``mode`` is "fibre" or "matrix".  Every routine carries complex
arithmetic through sigma and the polynomials and branches on the real part, so that the derivatives can be checked against complex
steps of the value in the state and in the table."""
import numpy as np

from ply_failure_ref import PlyFailureOracle

MODES = ("fibre", "matrix")


class PlyHashinOracle(PlyFailureOracle):
    mode = "fibre"

    def set_hashin_table(self, H):
        self.hsh = np.broadcast_to(np.asarray(H, dtype=np.float64), (self.mesh.nel, self.npt, 6)).copy()

    @staticmethod
    def coefficients(H):
        """(qt_f, qc_f, qt_m, qc_m, c1, sl), each shaped like H[..., 0]: FI = q s^2 (+ c1 s2) (+ sl t12^2) with q of the branch."""
        Xt, Xc, Yt, Yc, SL, ST = (H[..., k] for k in range(6))
        r = Yc / (2 * ST)
        return 1 / (Xt * Xt), 1 / (Xc * Xc), 1 / (Yt * Yt), 1 / (4 * ST * ST), (r * r - 1) / Yc, 1 / (SL * SL)

    @staticmethod
    def sigma_of(table, s):
        """sigma and x = eps - z kappa (nel, nq, npt, 3) from table (nel, npt, 16) and s (nel, nq, 6)."""
        G = table[:, :, 0:9].reshape(table.shape[0], -1, 3, 3)
        z = table[:, :, 9]
        x = s[:, :, None, 0:3] - z[:, None, :, None] * s[:, :, None, 3:6]
        return np.einsum("epij,eqpj->eqpi", G, x), x

    def _branch(self, sig, mode):
        """(a, b, sl, d): FI = a s_d^2 + b s_d + sl t12^2 on the (nel, nq, npt) grid of sig, d the component the sign is taken of;
        and the tension mask."""
        qtf, qcf, qtm, qcm, c1, sl = (c[:, None, :] for c in self.coefficients(self.hsh))
        if mode == "fibre":
            t = sig[..., 0].real >= 0
            return np.where(t, qtf, qcf), np.zeros_like(t, dtype=float), np.zeros_like(t, dtype=float), 0, t
        if mode != "matrix":
            raise ValueError(mode)
        t = sig[..., 1].real >= 0
        return np.where(t, qtm, qcm), np.where(t, 0.0, c1), np.broadcast_to(sl, t.shape), 1, t

    def _fi(self, sig, mode):
        a, b, sl, d, t = self._branch(sig, mode)
        sd, t12 = sig[..., d], sig[..., 2]
        return a * sd * sd + b * sd + sl * t12 * t12, t

    def indices(self, w, table=None):
        """(FI_f, FI_m, tension mask of s1, tension mask of s2), each (nel, nq, npt)."""
        s = self.strains(w)[0]
        sig, _ = self.sigma_of(self.ply if table is None else table, s)
        ff, tf = self._fi(sig, "fibre")
        fm, tm = self._fi(sig, "matrix")
        return ff, fm, tf, tm

    def failure_index(self, w, table=None):
        s, wj, wd, _ = self.strains(w)
        sig, _ = self.sigma_of(self.ply if table is None else table, s)
        return self._fi(sig, self.mode)[0], wj, wd

    def field(self, w):
        """(fibre, matrix), each (nel, npt): max over the quadrature points."""
        ff, fm, _, _ = self.indices(w)
        return ff.max(axis=1), fm.max(axis=1)

    def value(self, w, rho, mode, **kw):
        self.mode = mode
        return super().value(w, rho, **kw)

    def _dsig(self, sig, mode, c):
        """c dFI / dsigma (..., 3) on the (nel, nq, npt) grid."""
        a, b, sl, d, _ = self._branch(sig, mode)
        sb = np.zeros(sig.shape, dtype=np.result_type(sig, c))
        sb[..., d] = c * (2 * a * sig[..., d] + b)
        sb[..., 2] = c * 2 * sl * sig[..., 2]
        return sb

    def _pull(self, table, s, B, sb, x):
        """(d / d w (ndof), d / d table (nel, npt, 16)) from sbar = d / dsigma (nel, nq, npt, 3)."""
        nel, npt = table.shape[0], table.shape[1]
        G = table[:, :, 0:9].reshape(nel, npt, 3, 3)
        z = table[:, :, 9]
        xb = np.einsum("epij,eqpi->eqpj", G, sb)
        sbar = np.concatenate([xb.sum(axis=2), -(z[:, None, :, None] * xb).sum(axis=2)], axis=-1)
        ge = np.einsum("eqik,eqi->ek", B, sbar)
        gw = np.zeros(self.mesh.ndof)
        np.add.at(gw, self.dofs.ravel(), ge.ravel())
        gt = np.zeros((nel, npt, 16))
        gt[:, :, 0:9] = np.einsum("eqpi,eqpj->epij", sb, x).reshape(nel, npt, 9)
        gt[:, :, 9] = -np.einsum("eqpj,eqj->ep", xb, s[:, :, 3:6])
        return gw, gt

    def gradients(self, w, rho, mode, cells=None):
        """(dK/dw (ndof), dK/dtable (nel, npt, 16)); the columns 10..15 are zero."""
        s, wj, wd, B = self.strains(w)
        sig, x = self.sigma_of(self.ply, s)
        fi, _ = self._fi(sig, mode)
        sel = self._cells(cells)
        u = rho * fi
        shift = np.max(u[sel])
        c = wj[:, :, None] * np.exp(u - shift) * sel[:, None, None]
        c = c / c.sum()                                              # dK / dFI_eqp
        return self._pull(self.ply, s, B, self._dsig(sig, mode, c), x)

    def maximisers(self, w, mode, table=None):
        """(nel, npt): the first quadrature point that attains the maximum."""
        s = self.strains(w)[0]
        sig, _ = self.sigma_of(self.ply if table is None else table, s)
        return self._fi(sig, mode)[0].argmax(axis=1)

    def field_vjp(self, w, cbar, mode, table=None):
        """((d field / d w)^T cbar (ndof), (d field / d table)^T cbar (nel, npt, 16)) for cbar (nel, npt): the derivative of the index
        at the first quadrature point that attains the maximum."""
        table = self.ply if table is None else table
        nel, npt = table.shape[0], table.shape[1]
        s, _, _, B = self.strains(w)
        sig, x = self.sigma_of(table, s)
        qmax = self._fi(sig, mode)[0].argmax(axis=1)
        c = np.zeros(sig.shape[:3])
        c[np.arange(nel)[:, None], qmax, np.arange(npt)[None, :]] = np.asarray(cbar).reshape(nel, npt)
        return self._pull(table, s, B, self._dsig(sig, mode, c), x)
