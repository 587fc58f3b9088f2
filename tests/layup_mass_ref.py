"""CPU reference of the layup's mass and volume (include/femo_hip.h, femo_set_layup_density), numpy only, written from the contract:

    layup_mass   = sum_e (sum_k rho_k t_ek) W_e,    layup_volume = sum_e (sum_k t_ek) W_e,    W_e = sum_q w_q det_q J_q(uhat)

over a set of cells, with det, J(uhat) and the weights of the oracle's geometry at its full rule (``ShellOracle._geometry``), the way
tests/ply_failure_ref.py takes them.  d / d t_ek = rho_k W_e (or W_e) inside the set and zero outside it."""
import numpy as np

from oracle.rm_shell_oracle import ShellOracle


class LayupMassRef:
    def __init__(self, mesh, uhat=None, nquad=None):
        self.mesh = mesh
        self.o = ShellOracle(mesh, nquad=nquad)
        self.set_uhat(uhat)

    def set_uhat(self, uhat=None):
        self.o.set_fields(uhat=np.zeros((self.mesh.nn, 3)) if uhat is None else uhat)

    def _cells(self, cells):
        return np.ones(self.mesh.nel, bool) if cells is None else np.isin(np.arange(self.mesh.nel), np.asarray(cells))

    def cell_measure(self):
        """(nel,): W_e = sum_q w_q det_q J_q(uhat)."""
        o = self.o
        W = []
        for sl in o._chunks():
            g = o._geometry(sl, o.N1, o.dN1)
            W.append(np.sum(o.wts[None, :] * g["det"] * g["Ju"], axis=1))
        return np.concatenate(W)

    @staticmethod
    def _areal(t, rho):
        t = np.asarray(t, dtype=np.float64)
        return t.sum(axis=1) if rho is None else t @ np.asarray(rho, dtype=np.float64)

    def value(self, t, rho=None, cells=None):
        """layup_mass (``rho``: the (nply,) densities) or layup_volume (``rho`` None) of the (nel, nply) thicknesses ``t``."""
        return float(np.sum((self._areal(t, rho) * self.cell_measure())[self._cells(cells)]))

    def dthickness(self, nply, rho=None, cells=None):
        """(nel, nply): the gradient with respect to the ply thicknesses."""
        r = np.ones(nply) if rho is None else np.asarray(rho, dtype=np.float64)
        return (self.cell_measure() * self._cells(cells))[:, None] * r[None, :]
