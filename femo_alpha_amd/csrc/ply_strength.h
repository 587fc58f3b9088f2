// Load-proportional ply strength index of laminated shells (the inverse strength ratio / reserve factor of the Tsai-Wu criterion),
// aggregate and field, gfx950, fp64.  Reads the ply table of ply_failure.h unchanged.
//
// With sigma = G (eps - z kappa) of ply_fi at quadrature point q of the degree-4 stress measure and recovery point p of cell e:
//   b = F1 s1 + F2 s2,    a = F11 s1^2 + F22 s2^2 + F66 t12^2 + 2 F12 s1 s2        (FI = a + b)
//   D = sqrt(max(b^2 + 4 a, 0))
//   r = (b + D) / 2 for b >= 0,   r = 2 a / (D - b) for b < 0 (the same root without cancellation),   r = 0 where D = 0:
// the positive root of a / r^2 + b / r = 1, so the load may grow by 1 / r until first-ply failure and r(s w) = s r(w).  It needs
// a >= 0: the table's quadratic form is positive semidefinite (k_ply_psd_check; the library refuses any other table for these
// outputs).  Differentiating r^2 - b r - a = 0:
//   dr = (r db + da) / D,   defined as 0 where D = 0 (the apex of the cone, an unloaded point)
//   dr / dsigma = (r (F1, F2, 0) + da / dsigma) / D,    dr / d(F1, F2, F11, F22, F66, F12) = (r s1, r s2, s1^2, s2^2, t12^2, 2 s1 s2) / D;
// G and z enter through sigma as in PF_DTABLE.
//   S = log sum_e sum_q wj_q sum_p exp(rho r_eqp),    K = (S - log(alpha npt)) / rho,    dK / dr_eqp = wj_q exp(rho r_eqp - S).
// The reference has no ply recovery: this is the project's own contract, pinned by tests/ply_strength_ref.py.
//
// The layout is k_ply_failure's: one thread per cell, one wave per block; the six strains of every quadrature point are formed once
// and parked in the thread's own column of LDS (rolled loop, no barrier: columns are private), come back into registers, and the
// recovery points stream through them, p outermost, so that every entry of the entry-major table is read once.
//   PSI_VALUE   running pairs (m, z) = (max u, sum wj exp(u - m)), u = rho r; wave butterfly, one slot (m, z, reference area) per
//               block, merged in block order by k_ply_combine.  No atomics.
//   PSI_FIELD   out[e npt + p] = max_q r (every cell, whatever the selected sub-domain); the first maximiser in quadrature order
//               wins and a NaN stays visible (the update of PF_FIELD)
//   PSI_DW      strain cotangents per quadrature point first, then ONE strains_T_q per point; the element vector goes to the
//               cell's slot of ybuf for k_gather_sum (fixed order, no atomics)
//   PSI_DTABLE  every cell writes its own 16 npt row (cell-major, the layout of the ABI); zeros outside the selection
// The gradient modes take a cotangent cbar (nel npt, cell-major) or null.  Null: the aggregate, coefficient wj_q exp(rho r - S) at
// every q, S read from device memory (res[0] of k_ply_combine).  Given: the reverse mode of the field, coefficient cbar_ep at the
// maximiser q* alone, every cell live.  What the derivative needs at q* travels with the maximum through selects over the unrolled
// q, as in ply_field_rev.h; the strain cotangents are then summed in the thread's LDS column at the run-time index q*.  Nothing
// indexes a register array at run time.
#pragma once
#include "shell_device.h"
#include "stress_grad.h"
#include "ply_failure.h"
#include "ply_field_rev.h"

namespace femo {

enum { PSI_VALUE = 0, PSI_FIELD = 1, PSI_DW = 2, PSI_DTABLE = 3 };

// s: (e00, e11, g01, k00, k11, k01) of the point; x = eps - z kappa, sig = G x; returns r, and iD = 1 / D (0 where D = 0)
__device__ __forceinline__ double ply_sri(const PlyPoint& P, const double* s, double* x, double* sig, double& iD) {
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = s[j] - P.z * s[3 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) sig[i] = P.G[i][0] * x[0] + P.G[i][1] * x[1] + P.G[i][2] * x[2];
    const double b = P.F1 * sig[0] + P.F2 * sig[1];
    const double a = P.F11 * sig[0] * sig[0] + P.F22 * sig[1] * sig[1] + P.F66 * sig[2] * sig[2] + 2.0 * P.F12 * sig[0] * sig[1];
    const double t = b * b + 4.0 * a;
    const double D = sqrt(t < 0.0 ? 0.0 : t);                // a NaN passes through
    iD = D > 0.0 ? 1.0 / D : 0.0;
    const double r = b >= 0.0 ? 0.5 * (b + D) : 2.0 * a / (D - b);
    return D == 0.0 ? 0.0 : r;
}

// c dr / d sigma
__device__ __forceinline__ void ply_dsri(const PlyPoint& P, const double* sig, double r, double iD, double c, double* sb) {
    const double ci = c * iD;
    sb[0] = ci * (r * P.F1 + 2.0 * (P.F11 * sig[0] + P.F12 * sig[1]));
    sb[1] = ci * (r * P.F2 + 2.0 * (P.F22 * sig[1] + P.F12 * sig[0]));
    sb[2] = ci * 2.0 * P.F66 * sig[2];
}

// a += c dr / d(G, z, F1, F2, F11, F22, F66, F12) at one point (x = eps - z kappa, kap = kappa)
__device__ __forceinline__ void ply_dsri_dtable(const PlyPoint& P, const double* sig, const double* x, const double* kap, double r, double iD,
                                                double c, double* a) {
    double sb[3];
    ply_dsri(P, sig, r, iD, c, sb);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) a[3 * i + j] += sb[i] * x[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) a[9] -= (P.G[0][j] * sb[0] + P.G[1][j] * sb[1] + P.G[2][j] * sb[2]) * kap[j];
    const double ci = c * iD;
    a[10] += ci * r * sig[0];
    a[11] += ci * r * sig[1];
    a[12] += ci * sig[0] * sig[0];
    a[13] += ci * sig[1] * sig[1];
    a[14] += ci * sig[2] * sig[2];
    a[15] += 2.0 * ci * sig[0] * sig[1];
}

// the maximiser q* of r over the points' strains s (the update of PSI_FIELD), with r, 1 / D, sigma, x and kappa at q*
template <int NQ>
__device__ __forceinline__ int ply_sri_maximiser(const PlyPoint& P, const double (&s)[NQ][6], double& rm, double& iDm, double* sigm, double* xm,
                                                 double* km) {
    double mx = -INFINITY;
    int qs = 0;
    iDm = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) sigm[j] = xm[j] = km[j] = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double x[3], sig[3], iD;
        const double r = ply_sri(P, s[q], x, sig, iD);
        const bool take = r > mx || r != r;                  // the first point in quadrature order wins; a NaN stays visible
        mx = take ? r : mx;
        qs = take ? q : qs;
        iDm = take ? iD : iDm;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            sigm[j] = take ? sig[j] : sigm[j];
            xm[j] = take ? x[j] : xm[j];
            km[j] = take ? s[q][3 + j] : km[j];
        }
    }
    rm = mx;
    return qs;
}

// res: shift S of the aggregate's gradient modes (read when cbar is null); cbar: cotangent of the field (nel npt) or null; eslot: slot
// of every cell in ybuf (PSI_DW); out: part (PSI_VALUE, 3 doubles per block), the field (PSI_FIELD), ybuf (PSI_DW), d / d table
// (PSI_DTABLE).  m selects the sub-domain: the caller passes every cell with a cotangent.
template <int NPC, int NVC, bool QUAD, bool UHAT, int MODE>
__global__ void __launch_bounds__(PLY_BLOCK)
k_ply_strength(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ plyT, int npt, double rho,
               const double* __restrict__ w, const double* __restrict__ res, const double* __restrict__ cbar, const int* __restrict__ eslot,
               double* __restrict__ out) {
    constexpr int LD = 3 * NPC + 3 * NVC, NQ = QUAD ? 9 : 6;
    constexpr int ROWS = MODE == PSI_FIELD ? 6 : 7;         // per quadrature point: the strains, and the weight where a mode needs it
    __shared__ double s_q[ROWS * NQ][PLY_BLOCK];
    const int tid = threadIdx.x, e = blockIdx.x * PLY_BLOCK + tid;
    const bool live = e < m.nel && (MODE == PSI_FIELD || cell_selected(m, e));
    double km = -INFINITY, kz = 0.0, area = 0.0;
    if (live) {
        Elem<NPC, NVC> el;
        load_elem<NPC, NVC, UHAT>(m, f, e, el);
        double s[NQ][6], wj[NQ];
        if constexpr (MODE == PSI_FIELD) ply_point_strains<NPC, NVC, QUAD, UHAT, NQ>(m, tab, el, w, s_q, tid, s);
        else area = ply_point_strains_w<NPC, NVC, QUAD, UHAT, NQ>(m, tab, el, w, s_q, tid, s, wj);
        if constexpr (MODE == PSI_FIELD) {
            for (int p = 0; p < npt; ++p) {
                PlyPoint P;
                load_ply(plyT, m.nel, e, p, P);
                double mx = -INFINITY;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double x[3], sig[3], iD;
                    const double r = ply_sri(P, s[q], x, sig, iD);
                    mx = r > mx || r != r ? r : mx;
                }
                out[(size_t)e * npt + p] = mx;
            }
        } else if constexpr (MODE == PSI_VALUE) {
            for (int p = 0; p < npt; ++p) {
                PlyPoint P;
                load_ply(plyT, m.nel, e, p, P);
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double x[3], sig[3], iD;
                    ks_push_w(km, kz, rho * ply_sri(P, s[q], x, sig, iD), wj[q]);
                }
            }
        } else if constexpr (MODE == PSI_DW) {
            // the strains are in registers: the column now collects the strain cotangents per quadrature point
            if (cbar) {
                for (int i = 0; i < 7 * NQ; ++i) s_q[i][tid] = 0.0;
                const double* __restrict__ cb = cbar + (size_t)e * npt;
                for (int p = 0; p < npt; ++p) {
                    PlyPoint P;
                    load_ply(plyT, m.nel, e, p, P);
                    double rm, iDm, sigm[3], xm[3], kpm[3], sb[3];
                    const int qs = ply_sri_maximiser<NQ>(P, s, rm, iDm, sigm, xm, kpm);
                    ply_dsri(P, sigm, rm, iDm, cb[p], sb);
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const double t = P.G[0][j] * sb[0] + P.G[1][j] * sb[1] + P.G[2][j] * sb[2];
                        s_q[7 * qs + j][tid] += t;
                        s_q[7 * qs + 3 + j][tid] -= P.z * t;
                    }
                }
            } else {
                const double sh = res[0];
                double eb[NQ][3], kb[NQ][3];
#pragma unroll
                for (int q = 0; q < NQ; ++q)
#pragma unroll
                    for (int j = 0; j < 3; ++j) eb[q][j] = kb[q][j] = 0.0;
                for (int p = 0; p < npt; ++p) {
                    PlyPoint P;
                    load_ply(plyT, m.nel, e, p, P);
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        double x[3], sig[3], sb[3], iD;
                        const double r = ply_sri(P, s[q], x, sig, iD);
                        ply_dsri(P, sig, r, iD, wj[q] * exp(rho * r - sh), sb);
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            const double t = P.G[0][j] * sb[0] + P.G[1][j] * sb[1] + P.G[2][j] * sb[2];
                            eb[q][j] += t;
                            kb[q][j] -= P.z * t;
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q)
#pragma unroll
                    for (int j = 0; j < 3; ++j) { s_q[7 * q + j][tid] = eb[q][j]; s_q[7 * q + 3 + j][tid] = kb[q][j]; }
            }
            ply_strain_cotangents_to_ybuf<NPC, NVC, QUAD, UHAT, NQ>(tab, el, s_q, tid, eslot, e, out);
        } else {
            const double sh = cbar ? 0.0 : res[0];
            for (int p = 0; p < npt; ++p) {
                PlyPoint P;
                load_ply(plyT, m.nel, e, p, P);
                double a[PLY_W];
#pragma unroll
                for (int k = 0; k < PLY_W; ++k) a[k] = 0.0;
                if (cbar) {
                    double rm, iDm, sigm[3], xm[3], kpm[3];
                    ply_sri_maximiser<NQ>(P, s, rm, iDm, sigm, xm, kpm);
                    ply_dsri_dtable(P, sigm, xm, kpm, rm, iDm, cbar[(size_t)e * npt + p], a);
                } else {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        double x[3], sig[3], iD;
                        const double r = ply_sri(P, s[q], x, sig, iD);
                        ply_dsri_dtable(P, sig, x, &s[q][3], r, iD, wj[q] * exp(rho * r - sh), a);
                    }
                }
                double* o = out + ((size_t)e * npt + p) * PLY_W;
#pragma unroll
                for (int k = 0; k < PLY_W; ++k) o[k] = a[k];
            }
        }
    } else if (e < m.nel) {                      // outside the selected sub-domain
        if constexpr (MODE == PSI_DW) ply_zero_ybuf_slot<LD>(eslot, e, out);
        else if constexpr (MODE == PSI_DTABLE) ply_zero_table_row<PLY_W>(e, npt, out);
    }
    if constexpr (MODE == PSI_VALUE) ply_block_slot(km, kz, area, tid, out);
}

// The quadratic form of every recovery point must be positive semidefinite for r to exist: F11, F22, F66 >= 0 and
// F12^2 <= F11 F22 (1 + 1e-12) (the slack covers the rounding of tsai_wu(f12 = +-1)).  tab: the cell-major table.  *first (set to
// INT_MAX by the caller) receives the smallest offending index e npt + p: an integer minimum, whose result does not depend on order.
__global__ void __launch_bounds__(256)
k_ply_psd_check(const double* __restrict__ tab, long long npoints, int* __restrict__ first) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npoints) return;
    const double* P = tab + (size_t)i * PLY_W;
    const double F11 = P[12], F22 = P[13], F66 = P[14], F12 = P[15];
    const bool ok = F11 >= 0.0 && F22 >= 0.0 && F66 >= 0.0 && F12 * F12 <= F11 * F22 * (1.0 + 1e-12);
    if (!ok) atomicMin(first, (int)i);
}

}  // namespace femo
