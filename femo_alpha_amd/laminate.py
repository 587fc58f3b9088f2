"""Laminate stiffness for the composite shell law (host numpy; ``ShellContext.set_laminate`` / ``femo_set_laminate``).

The reference's ``MaterialModelComposite`` takes per-cell CLT matrices ``A``, ``B``, ``D`` (3 x 3) and ``A_s`` (2 x 2)
(femo_alpha/rm_shell/linear_shell_fenicsx/linear_shell_model.py:159-190) and leaves their computation to the caller.  This module is
that caller-side step: classical lamination theory from orthotropic plies, a rotation in the element plane, and the 32-wide packing of
the C ABI.

Conventions (include/femo_hip.h, femo_set_laminate):
  * Voigt strains eps = (e00, e11, 2 e01), kappa = (k00, k11, 2 k01), gamma = (g0, g1) in the local frame of every point:
    laminate axis 1 lies along E0, from vertex 0 toward vertex 1 of the cell.
  * Plies are listed bottom to top (z from -H/2 to H/2 along the cell normal by default); angles in degrees, measured from E0 toward
    E1.
  * ``A_s = K_SHEAR * sum_k Qs_k t_k`` with the project's shear correction 0.833, so one isotropic ply of thickness h gives the
    single-layer law: (h C, 0, h^3 / 12 C, 0.833 G h I).
  * The strain at height z above the reference surface is eps - z kappa (u(z) = u_mid - z E2 x theta, linear_shell_model.py:392-398),
    so B = -int z Qbar dz: a ply above the mid-surface contributes a negative B.
  * A reference-plane offset -- the mid-surface o above the reference surface (the reference's ``shl_offset``; its single layer on
    top of the reference surface, ``getSingleLayerCLT`` with BOT, is o = h / 2) -- is the transform A' = A, B' = B - o A,
    D' = D - o (B + B^T) + o^2 A (``offset``).  ``clt_from_plies``, ``clt_dtheta`` and ``ply_table`` build about such a surface
    directly (``reference``, ``offset``: o = r H + c, ``_interfaces``), with the thickness Jacobians of the shift included; the device
    counterpart is femo_set_layup_reference.
"""
from __future__ import annotations

import numpy as np

K_SHEAR = 0.833          # linear_shell_model.py:146
LAM_W = 32               # [A (9), B (9), D (9), A_s (4), c_drill] per cell
PLY_W = 16               # [G (9), z, F1, F2, F11, F22, F66, F12] per recovery point (femo_set_ply_table)
PSH_W = 6                # [Gs (4), F55, F44] per recovery point (femo_set_ply_shear_table)
HSH_W = 6                # [Xt, Xc, Yt, Yc, SL, ST] per recovery point (femo_set_ply_hashin_table)


def _t_eps(theta_deg):
    """Strain transformation eps_ply = T(theta) eps_frame of the in-plane Voigt strains (engineering shear), (..., 3, 3)."""
    th = np.deg2rad(np.asarray(theta_deg, dtype=np.float64))
    m, n = np.cos(th), np.sin(th)
    T = np.empty(th.shape + (3, 3))
    T[..., 0, 0], T[..., 0, 1], T[..., 0, 2] = m * m, n * n, m * n
    T[..., 1, 0], T[..., 1, 1], T[..., 1, 2] = n * n, m * m, -m * n
    T[..., 2, 0], T[..., 2, 1], T[..., 2, 2] = -2 * m * n, 2 * m * n, m * m - n * n
    return T


def _r_shear(theta_deg):
    """gamma_ply = R(theta) gamma_frame of the transverse shear strains, (..., 2, 2)."""
    th = np.deg2rad(np.asarray(theta_deg, dtype=np.float64))
    m, n = np.cos(th), np.sin(th)
    R = np.empty(th.shape + (2, 2))
    R[..., 0, 0], R[..., 0, 1], R[..., 1, 0], R[..., 1, 1] = m, n, -n, m
    return R


def ply_stiffness(E1, E2, G12, nu12, G13, G23, theta):
    """Reduced stiffness Qbar (..., 3, 3) and transverse shear stiffness Qs (..., 2, 2) of plies rotated by ``theta`` degrees."""
    E1, E2, G12, nu12, G13, G23 = (np.asarray(x, dtype=np.float64) for x in (E1, E2, G12, nu12, G13, G23))
    shape = np.broadcast(E1, E2, G12, nu12, G13, G23, np.asarray(theta)).shape
    nu21 = nu12 * E2 / E1
    den = 1.0 - nu12 * nu21
    Q = np.zeros(shape + (3, 3))
    Q[..., 0, 0] = E1 / den
    Q[..., 1, 1] = E2 / den
    Q[..., 0, 1] = Q[..., 1, 0] = nu12 * E2 / den
    Q[..., 2, 2] = G12
    Qs = np.zeros(shape + (2, 2))
    Qs[..., 0, 0], Qs[..., 1, 1] = G13, G23
    T = np.broadcast_to(_t_eps(theta), shape + (3, 3))
    R = np.broadcast_to(_r_shear(theta), shape + (2, 2))
    Qbar = np.einsum("...ki,...kl,...lj->...ij", T, Q, T)
    Qsbar = np.einsum("...ki,...kl,...lj->...ij", R, Qs, R)
    return Qbar, Qsbar


def clt_from_plies(E1, E2, G12, nu12, G13, G23, t, theta, k_shear=K_SHEAR, jacobian=False, reference="mid", offset=0.0):
    """Classical lamination theory.  Every argument is an array of shape (nply,) (one layup for all cells) or (nel, nply); plies bottom
    to top, ``theta`` in degrees from E0.  Returns (A, B, D, A_s) of shapes (nel, 3, 3) x 3 and (nel, 2, 2) (nel = 1 for a single
    layup); with ``jacobian=True`` also (dA, dB, dD, dA_s), the derivatives with respect to the ply thicknesses, shapes
    (nel, nply, 3, 3) x 3 and (nel, nply, 2, 2) -- the chain from d/d laminate to d/d t.
    ``reference`` / ``offset``: the reference surface the laminate is built about (``_interfaces``); the default is the
    mid-surface.  ``offset`` is data: the Jacobians differentiate the thickness-dependent part r H of the shift only."""
    args = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (E1, E2, G12, nu12, G13, G23, t, theta)]
    args = np.broadcast_arrays(*args)
    E1, E2, G12, nu12, G13, G23, t, theta = args
    Qb, Qs = ply_stiffness(E1, E2, G12, nu12, G13, G23, theta)          # (nel, nply, 3, 3), (nel, nply, 2, 2)
    z = _interfaces(t, reference, offset)                                             # (nel, nply + 1) ply interfaces
    z0, z1 = z[:, :-1], z[:, 1:]
    A = np.einsum("ek,ekij->eij", z1 - z0, Qb)
    # the strain at height z is eps - z kappa (u(z) = u_mid - z E2 x theta, linear_shell_model.py:392-398): B = -int z Qbar dz
    B = -0.5 * np.einsum("ek,ekij->eij", z1 ** 2 - z0 ** 2, Qb)
    D = np.einsum("ek,ekij->eij", z1 ** 3 - z0 ** 3, Qb) / 3.0
    As = k_shear * np.einsum("ek,ekij->eij", t, Qs)
    if not jacobian:
        return A, B, D, As
    nply = t.shape[1]
    dz = _dz_interfaces(nply, reference)                                                          # (nply + 1, nply) [i, j]
    dz0, dz1 = dz[:-1], dz[1:]                                                                    # (nply, nply) [k, j]
    dA = np.einsum("kj,ekab->ejab", dz1 - dz0, Qb)
    dB = np.einsum("ek,kj,ekab->ejab", z0, dz0, Qb) - np.einsum("ek,kj,ekab->ejab", z1, dz1, Qb)
    dD = np.einsum("ek,kj,ekab->ejab", z1 ** 2, dz1, Qb) - np.einsum("ek,kj,ekab->ejab", z0 ** 2, dz0, Qb)
    dAs = k_shear * Qs
    return (A, B, D, As), (dA, dB, dD, dAs)


REFERENCES = {"mid": 0.0, "bot": 0.5, "top": -0.5}


def reference_position(reference):
    """The number r of a reference surface: its position below the mid-surface in units of the cell's total thickness H.
    "mid" = 0, "bot" = 1/2, "top" = -1/2, or any finite number."""
    if isinstance(reference, str):
        if reference not in REFERENCES:
            raise ValueError(f"reference: 'mid', 'bot', 'top' or a number, got {reference!r}")
        return REFERENCES[reference]
    r = float(reference)
    if not np.isfinite(r):
        raise ValueError(f"reference: a finite number, got {reference!r}")
    return r


def _interfaces(t, reference="mid", offset=0.0):
    """The nply + 1 ply interfaces z_i = sum_{j < i} t_j - (1/2 - r) H + c of the (nel, nply) thicknesses ``t`` about the reference
    surface r = ``reference_position(reference)``, c = ``offset`` (a scalar or one length per cell), (nel, nply + 1).  The reference
    surface lies o = r H + c below the mid-surface (the ``o`` of ``offset``): "bot" has z_0 = c, "top" z_nply = c.  c is added only
    where it is given, so the default performs the operations of the mid-surface convention z_i = sum_{j < i} t_j - H / 2."""
    H = t.sum(axis=1, keepdims=True)
    z = np.concatenate([np.zeros_like(H), np.cumsum(t, axis=1)], axis=1) - (0.5 - reference_position(reference)) * H
    c = np.asarray(offset, dtype=np.float64)
    if c.ndim == 0 and c == 0.0:
        return z
    return z + (c.reshape(-1, 1) if c.ndim else c)


def _dz_interfaces(nply, reference="mid", offset=0.0):
    """dz_i / dt_j = [j < i] - (1/2 - r) of the nply + 1 ply interfaces of ``_interfaces``, (nply + 1, nply); ``offset`` is data and
    does not enter."""
    return -(0.5 - reference_position(reference)) + (np.arange(nply)[None, :] < np.arange(nply + 1)[:, None]).astype(np.float64)


def _dt_eps(theta_deg):
    """d T / d theta of ``_t_eps``, per radian, (..., 3, 3)."""
    th = np.deg2rad(np.asarray(theta_deg, dtype=np.float64))
    c2, s2 = np.cos(2 * th), np.sin(2 * th)
    dT = np.empty(th.shape + (3, 3))
    dT[..., 0, 0], dT[..., 0, 1], dT[..., 0, 2] = -s2, s2, c2
    dT[..., 1, 0], dT[..., 1, 1], dT[..., 1, 2] = s2, -s2, -c2
    dT[..., 2, 0], dT[..., 2, 1], dT[..., 2, 2] = -2 * c2, 2 * c2, -2 * s2
    return dT


def ply_stiffness_dtheta(E1, E2, G12, nu12, G13, G23, theta):
    """d Qbar / d theta (..., 3, 3) and d Qsbar / d theta (..., 2, 2) of ``ply_stiffness``, per degree."""
    E1, E2, G12, nu12, G13, G23 = (np.asarray(x, dtype=np.float64) for x in (E1, E2, G12, nu12, G13, G23))
    shape = np.broadcast(E1, E2, G12, nu12, G13, G23, np.asarray(theta)).shape
    Q, Qs = ply_stiffness(E1, E2, G12, nu12, G13, G23, np.zeros(shape))          # theta = 0: the ply-axis stiffnesses
    T = np.broadcast_to(_t_eps(theta), shape + (3, 3))
    dT = np.broadcast_to(_dt_eps(theta), shape + (3, 3))
    th = np.broadcast_to(np.deg2rad(np.asarray(theta, dtype=np.float64)), shape)
    m, n = np.cos(th), np.sin(th)
    R = np.broadcast_to(_r_shear(theta), shape + (2, 2))
    dR = np.empty(shape + (2, 2))
    dR[..., 0, 0], dR[..., 0, 1], dR[..., 1, 0], dR[..., 1, 1] = -n, m, -m, -n
    dQb = np.einsum("...ki,...kl,...lj->...ij", dT, Q, T) + np.einsum("...ki,...kl,...lj->...ij", T, Q, dT)
    dQs = np.einsum("...ki,...kl,...lj->...ij", dR, Qs, R) + np.einsum("...ki,...kl,...lj->...ij", R, Qs, dR)
    return np.deg2rad(1.0) * dQb, np.deg2rad(1.0) * dQs


def clt_dtheta(E1, E2, G12, nu12, G13, G23, t, theta, k_shear=K_SHEAR, reference="mid", offset=0.0):
    """(dA, dB, dD, dA_s): the derivatives of ``clt_from_plies`` with respect to the ply angles, per degree, shapes
    (nel, nply, 3, 3) x 3 and (nel, nply, 2, 2) -- entry [e, k] is the derivative with respect to the angle of ply k of cell e.
    Arguments as for ``clt_from_plies``, the reference surface included."""
    args = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (E1, E2, G12, nu12, G13, G23, t, theta)]
    E1, E2, G12, nu12, G13, G23, t, theta = np.broadcast_arrays(*args)
    dQb, dQs = ply_stiffness_dtheta(E1, E2, G12, nu12, G13, G23, theta)
    z = _interfaces(t, reference, offset)
    z0, z1 = z[:, :-1], z[:, 1:]
    w = lambda x: x[:, :, None, None]
    return w(z1 - z0) * dQb, -0.5 * w(z1 ** 2 - z0 ** 2) * dQb, w(z1 ** 3 - z0 ** 3) * dQb / 3.0, k_shear * w(t) * dQs


def ply_table_dtheta(E1, E2, G12, nu12, theta):
    """d G / d theta (nel, nply, 3, 3), per degree, of the G = Q T(theta) that ``ply_table`` stores at every recovery point of a
    ply: the only entries of the table that depend on the ply angles.  Ply arguments as for ``ply_table``."""
    args = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (E1, E2, G12, nu12, theta)]
    E1, E2, G12, nu12, theta = np.broadcast_arrays(*args)
    Q, _ = ply_stiffness(E1, E2, G12, nu12, G12, G12, np.zeros_like(theta))
    return np.deg2rad(1.0) * np.einsum("ekil,eklj->ekij", Q, _dt_eps(theta))


def tsai_wu(Xt, Xc, Yt, Yc, S, f12=-0.5):
    """The six coefficients (F1, F2, F11, F22, F66, F12) of the Tsai-Wu failure index
    FI = F1 s1 + F2 s2 + F11 s1^2 + F22 s2^2 + F66 t12^2 + 2 F12 s1 s2 from the ply strengths (all positive: tension / compression
    along and across the fibres, in-plane shear), F12 = f12 sqrt(F11 F22).  Arguments broadcast; the coefficients are the last axis.
    Xt = Xc = Yt = Yc = X, S = X / sqrt(3), f12 = -1/2 gives (von Mises / X)^2."""
    Xt, Xc, Yt, Yc, S, f12 = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (Xt, Xc, Yt, Yc, S, f12)))
    F11, F22 = 1.0 / (Xt * Xc), 1.0 / (Yt * Yc)
    return np.stack([1.0 / Xt - 1.0 / Xc, 1.0 / Yt - 1.0 / Yc, F11, F22, 1.0 / S ** 2, f12 * np.sqrt(F11 * F22)], axis=-1)


def ply_table(E1, E2, G12, nu12, t, theta, strengths, surfaces=("bot", "top"), jacobian=False, reference="mid", offset=0.0):
    """Recovery points of the ply failure outputs (femo_set_ply_table): (nel, npt, 16) with npt = nply * len(surfaces), per point
    [G (3x3 row-major), z, F1, F2, F11, F22, F66, F12].  Ply arguments as for ``clt_from_plies``: (nply,) or (nel, nply), plies bottom
    to top, z from -H/2; ``strengths``: the coefficients of ``tsai_wu``, (6,), (nply, 6) or (nel, nply, 6).  Point order: ply by ply
    from the bottom, inside a ply the ``surfaces`` as listed ("bot", "mid", "top" of the ply).  G = Q T(theta) maps the frame strains
    eps - z kappa to the ply-axis stresses (Q: the reduced stiffness in ply axes, T: ``_t_eps``).
    ``jacobian=True`` also returns dz (npt, nply) = d z_p / d t_j, the same for every cell: z is the only entry of the table that
    depends on the ply thicknesses.  ``reference`` / ``offset``: the reference surface z is measured from (``_interfaces``)."""
    args = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (E1, E2, G12, nu12, t, theta)]
    E1, E2, G12, nu12, t, theta = np.broadcast_arrays(*args)
    nel, nply = t.shape
    Q, _ = ply_stiffness(E1, E2, G12, nu12, G12, G12, np.zeros_like(theta))         # theta = 0: Q in ply axes
    G = np.einsum("ekil,eklj->ekij", Q, _t_eps(theta))
    F = np.broadcast_to(np.asarray(strengths, dtype=np.float64), (nel, nply, 6))
    z = _interfaces(t, reference, offset)                                             # (nel, nply + 1) ply interfaces
    dzi = _dz_interfaces(nply, reference)
    pick = {"bot": (1.0, 0.0), "mid": (0.5, 0.5), "top": (0.0, 1.0)}
    ns = len(surfaces)
    out = np.empty((nel, nply, ns, PLY_W))
    dz = np.empty((nply, ns, nply))
    for s, name in enumerate(surfaces):
        if name not in pick:
            raise ValueError(f"surfaces: 'bot', 'mid' or 'top', got {name!r}")
        a, b = pick[name]
        out[:, :, s, 0:9] = G.reshape(nel, nply, 9)
        out[:, :, s, 9] = a * z[:, :-1] + b * z[:, 1:]
        out[:, :, s, 10:16] = F
        dz[:, s, :] = a * dzi[:-1] + b * dzi[1:]
    out = out.reshape(nel, nply * ns, PLY_W)
    return (out, dz.reshape(nply * ns, nply)) if jacobian else out


def hashin_strengths(Xt, Xc, Yt, Yc, SL, ST=None):
    """The six strengths [Xt, Xc, Yt, Yc, SL, ST] of the Hashin fibre and matrix failure indices (femo_set_ply_hashin_table), all
    positive: tension / compression along and across the fibres, the longitudinal (in-plane) and the transverse shear strength.
    ``ST=None`` takes Yc / 2, for which the matrix index has no kink at s2 = 0.  Arguments broadcast; the strengths are the last
    axis.
        fibre   (s1/Xt)^2 for s1 >= 0, (s1/Xc)^2 for s1 < 0
        matrix  (s2/Yt)^2 + (t12/SL)^2 for s2 >= 0, (s2/(2 ST))^2 + ((Yc/(2 ST))^2 - 1) s2/Yc + (t12/SL)^2 for s2 < 0"""
    Yc = np.asarray(Yc, dtype=np.float64)
    vals = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (Xt, Xc, Yt, Yc, SL, 0.5 * Yc if ST is None else ST)))
    out = np.stack(vals, axis=-1)
    if not (np.all(np.isfinite(out)) and np.all(out > 0)):
        raise ValueError("hashin_strengths: the strengths must be finite and > 0")
    return out


def hashin_table(strengths, nel, nply=None, surfaces=("bot", "top")):
    """The strengths table of femo_set_ply_hashin_table, (nel, npt, 6), in the point order of ``ply_table``: ply by ply from the
    bottom, inside a ply the ``surfaces`` as listed.  ``strengths``: the array of ``hashin_strengths``, (6,), (nply, 6) or
    (nel, nply, 6); ``nply`` is needed with (6,) alone.  The strengths depend on neither thickness nor angle."""
    s = np.asarray(strengths, dtype=np.float64)
    if s.shape[-1] != HSH_W:
        raise ValueError(f"hashin_table: [Xt, Xc, Yt, Yc, SL, ST] on the last axis, got shape {s.shape}")
    if s.ndim == 1:
        if nply is None:
            raise ValueError("hashin_table: (6,) strengths need nply")
        s = s[None, :]
    nply = s.shape[-2] if nply is None else int(nply)
    s = np.broadcast_to(s, (int(nel), nply, HSH_W))
    return np.ascontiguousarray(np.repeat(s, len(surfaces), axis=1))


def shear_strength(S13, S23):
    """The two coefficients (F55, F44) = (1 / S13^2, 1 / S23^2) of the interlaminar shear failure index
    FI = F55 t13^2 + F44 t23^2 from the transverse shear strengths (positive).  Arguments broadcast; the coefficients are the last
    axis."""
    S13, S23 = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (S13, S23)))
    return np.stack([1.0 / S13 ** 2, 1.0 / S23 ** 2], axis=-1)


def ply_shear_table(G13, G23, theta, strengths):
    """Recovery points of the interlaminar shear outputs (femo_set_ply_shear_table): (nel, nply, 6), one point per ply,
    [Gs (2x2 row-major), F55, F44] with Gs = diag(G13, G23) R(theta) (R: ``_r_shear``), which maps the cell-mean transverse shear
    strains of the frame to the ply-axis stresses (t13, t23) -- the constitutive first-order-shear recovery, constant within a ply,
    so the ply thicknesses do not enter.  G13, G23, theta: (nply,) or (nel, nply), plies bottom to top; ``strengths``: the
    coefficients of ``shear_strength``, (2,), (nply, 2) or (nel, nply, 2)."""
    G13, G23, theta = np.broadcast_arrays(*(np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (G13, G23, theta)))
    nel, nply = theta.shape
    R = _r_shear(theta)
    out = np.empty((nel, nply, PSH_W))
    out[..., 0], out[..., 1] = G13 * R[..., 0, 0], G13 * R[..., 0, 1]
    out[..., 2], out[..., 3] = G23 * R[..., 1, 0], G23 * R[..., 1, 1]
    out[..., 4:6] = np.broadcast_to(np.asarray(strengths, dtype=np.float64), (nel, nply, 2))
    return out


def ply_shear_table_dtheta(G13, G23, theta):
    """d Gs / d theta (nel, nply, 2, 2), per degree, of the Gs = diag(G13, G23) R(theta) that ``ply_shear_table`` stores: the only
    entries of that table that depend on the ply angles (dR / dtheta = [[-n, m], [-m, -n]])."""
    G13, G23, theta = np.broadcast_arrays(*(np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (G13, G23, theta)))
    th = np.deg2rad(theta)
    m, n = np.cos(th), np.sin(th)
    d = np.empty(theta.shape + (2, 2))
    d[..., 0, 0], d[..., 0, 1] = -G13 * n, G13 * m
    d[..., 1, 0], d[..., 1, 1] = -G23 * m, -G23 * n
    return np.deg2rad(1.0) * d


def offset(clt, o):
    """(A, B, D, A_s) about a reference surface that lies ``o`` below the mid-surface the laminate was built about."""
    A, B, D, As = (np.asarray(x, dtype=np.float64) for x in clt)
    o = np.asarray(o, dtype=np.float64).reshape(-1, 1, 1) if np.ndim(o) else o
    return A, B - o * A, D - o * (B + np.swapaxes(B, -1, -2)) + o * o * A, As


def rotate_clt(clt, angle):
    """The laminate (A, B, D, A_s) turned by ``angle`` degrees in the element plane: every ply angle grows by ``angle``.
    ``angle``: a scalar or one value per cell."""
    A, B, D, As = (np.asarray(x, dtype=np.float64) for x in clt)
    T = _t_eps(angle)
    R = _r_shear(angle)
    rot = lambda X, M: np.einsum("...ki,...kl,...lj->...ij", M, X, M)
    return rot(A, T), rot(B, T), rot(D, T), rot(As, R)


def pack(A, B, D, As, c_drill=None):
    """The (nel, 32) array femo_set_laminate takes: [A, B, D (row-major), A_s, c_drill] per cell.  ``c_drill=None`` applies the
    reference's drilling coefficient alpha = 12 max(D) over all entries of all cells (linear_shell_model.py:284-296), a constant;
    a scalar or one value per cell is used as given (c_drill = E h^3 reproduces the single-layer law's drilling term)."""
    A, B, D = (np.asarray(x, dtype=np.float64).reshape(-1, 3, 3) for x in (A, B, D))
    As = np.asarray(As, dtype=np.float64).reshape(-1, 2, 2)
    nel = max(len(A), len(B), len(D), len(As))
    out = np.empty((nel, LAM_W))
    out[:, 0:9] = np.broadcast_to(A.reshape(-1, 9), (nel, 9))
    out[:, 9:18] = np.broadcast_to(B.reshape(-1, 9), (nel, 9))
    out[:, 18:27] = np.broadcast_to(D.reshape(-1, 9), (nel, 9))
    out[:, 27:31] = np.broadcast_to(As.reshape(-1, 4), (nel, 4))
    out[:, 31] = 12.0 * float(np.max(D)) if c_drill is None else np.broadcast_to(np.asarray(c_drill, dtype=np.float64), (nel,))
    return out


def unpack(clt):
    """(A, B, D, A_s, c_drill) of a (nel, 32) array."""
    c = np.asarray(clt, dtype=np.float64).reshape(-1, LAM_W)
    return (c[:, 0:9].reshape(-1, 3, 3), c[:, 9:18].reshape(-1, 3, 3), c[:, 18:27].reshape(-1, 3, 3), c[:, 27:31].reshape(-1, 2, 2),
            c[:, 31].copy())


def isotropic(h, E, nu, c_drill=None):
    """The per-cell laminate of one isotropic ply (thickness h, E, nu per cell): the single-layer law of the isotropic path;
    ``c_drill=None`` gives E h^3, which makes it reproduce that path's drilling term too."""
    h, E, nu = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64).ravel() for x in (h, E, nu)))
    G = E / (2 * (1 + nu))
    A, B, D, As = clt_from_plies(E[:, None], E[:, None], G[:, None], nu[:, None], G[:, None], G[:, None], h[:, None],
                                 np.zeros((len(h), 1)))
    return pack(A, B, D, As, E * h ** 3 if c_drill is None else c_drill)
