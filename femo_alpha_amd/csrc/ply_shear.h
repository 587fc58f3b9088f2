// Interlaminar (transverse) shear failure aggregate and field of laminated shells (laminate mode, include/femo_hip.h:
// femo_set_ply_shear_table), gfx950, fp64.
//
// Per cell npt_s recovery points of PSH_W = 6 doubles [Gs (2x2 row-major), F55, F44].  With q over the degree-4 rule (Tables of the
// stress measure), wj_q = w_q det_q Ju_q and (ga0, ga1)_q the transverse shear strains of strains_q:
//   a_e = sum_q wj_q,    gbar_e = (1 / a_e) sum_q wj_q (ga0, ga1)_q        the CELL-MEAN shear strain
//   (t13, t23)_ep = Gs_ep gbar_e,    FI_ep = F55 t13^2 + F44 t23^2
//   S = log sum_e a_e sum_p exp(rho FI_ep),    K = (S - log(alpha npt_s)) / rho,    dK / dFI_ep = c_ep = a_e exp(rho FI_ep - S).
// Pointwise shear strains of the CG2 x CG1 element are off by tens of per cent on thin skins while the cell mean reaches the closed
// form to 1e-9 (README, "interlaminar shear"), hence the mean: one smooth number per (cell, point), no maximum over quadrature
// points, no tie to break.  The reference has no ply recovery: this is the project's own contract, pinned by tests/ply_shear_ref.py.
//
// One thread per cell, one wave per block, as k_ply_failure.  ONE pass over the quadrature points accumulates a_e and sum wj gamma --
// three doubles, nothing is parked in LDS; PS_VALUE alone adds the reference area for alpha -- and only the two shear strains are
// formed (shear_q).  The recovery points are then streamed, p outermost; the device table is entry-major ([6 p + k][nel]): the 64
// cells of a wave read 512 contiguous bytes per entry, every entry once.
//   PS_VALUE   running pairs (m, z) = (max u, sum a_e exp(u - m)), u = rho FI, merged over the wave by a butterfly, one slot
//              (m, z, reference area) per block; the slots are merged in block order by k_ply_combine (ply_failure.h).  No atomics.
//   PS_FIELD   out[e npt + p] = FI_ep (every cell, whatever the selected sub-domain)
//   PS_DW      dK / dgbar = sum_p Gs^T dK / dt is summed over the recovery points first; a second pass over the quadrature points
//              (geometry again) pushes (wj_q / a_e) of it through the shear-only transpose shear_T_q.  The cell's element vector goes
//              to its slot of ybuf for k_gather_sum (fixed order, no atomics).
//   PS_DTABLE  every cell writes its own 6 npt row [outer(dK / dt, gbar), c t13^2, c t23^2] (cell-major, the layout of the ABI); zeros
//              outside the selection.
// The coefficient c_ep of the gradient modes is the KS weight above (the shift S read from res[0] of k_ply_combine), or, with a
// cotangent cbar (nel npt, cell-major), cbar_ep itself: the reverse mode of the field, a mode of the same kernels.
#pragma once
#include "shell_device.h"
#include "ply_failure.h"

namespace femo {

constexpr int PSH_W = 6;           // doubles per recovery point
enum { PS_VALUE = 0, PS_FIELD = 1, PS_DW = 2, PS_DTABLE = 3 };

struct ShearPoint {
    double G[2][2], F55, F44;
};

// recovery point p of cell e from the entry-major device table
__device__ __forceinline__ void load_shear(const double* __restrict__ T, int nel, int e, int p, ShearPoint& P) {
    const double* s = T + (size_t)p * PSH_W * nel + e;
    P.G[0][0] = s[0];
    P.G[0][1] = s[(size_t)nel];
    P.G[1][0] = s[(size_t)2 * nel];
    P.G[1][1] = s[(size_t)3 * nel];
    P.F55 = s[(size_t)4 * nel];
    P.F44 = s[(size_t)5 * nel];
}

// the two transverse shear strains of strains_q, nothing else:  ga0 = theta . E1 + E2 . d_0 u,  ga1 = -theta . E0 + E2 . d_1 u
template <int NPC, int NVC>
__device__ __forceinline__ void shear_q(const Tables& t, int q, const QPG& g, const double* xe, double& ga0, double& ga1) {
    double g0 = 0.0, g1 = 0.0;
#pragma unroll
    for (int a = 0; a < NPC; ++a) {
        const double r0 = t.dN2[q][a][0], r1 = t.dN2[q][a][1];
        const double d0 = r0 * g.Q[0][0] + r1 * g.Q[1][0], d1 = r0 * g.Q[0][1] + r1 * g.Q[1][1];
        const double un = xe[3 * a] * g.E2[0] + xe[3 * a + 1] * g.E2[1] + xe[3 * a + 2] * g.E2[2];
        g0 += d0 * un;
        g1 += d1 * un;
    }
    double th[3] = {0, 0, 0};
#pragma unroll
    for (int b = 0; b < NVC; ++b) {
        const double Mb = t.NR[q][b];
#pragma unroll
        for (int c = 0; c < 3; ++c) th[c] += Mb * xe[3 * NPC + 3 * b + c];
    }
    ga0 = dot3(th, g.E1) + g0;
    ga1 = -dot3(th, g.E0) + g1;
}

// ye += B_q[ga0, ga1]^T (b0, b1): the transpose of shear_q
template <int NPC, int NVC>
__device__ __forceinline__ void shear_T_q(const Tables& t, int q, const QPG& g, double b0, double b1, double* ye) {
#pragma unroll
    for (int a = 0; a < NPC; ++a) {
        const double r0 = t.dN2[q][a][0], r1 = t.dN2[q][a][1];
        const double d0 = r0 * g.Q[0][0] + r1 * g.Q[1][0], d1 = r0 * g.Q[0][1] + r1 * g.Q[1][1];
        const double s = d0 * b0 + d1 * b1;
#pragma unroll
        for (int c = 0; c < 3; ++c) ye[3 * a + c] += s * g.E2[c];
    }
    double Tq[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) Tq[c] = b0 * g.E1[c] - b1 * g.E0[c];
#pragma unroll
    for (int b = 0; b < NVC; ++b) {
        const double Mb = t.NR[q][b];
#pragma unroll
        for (int c = 0; c < 3; ++c) ye[3 * NPC + 3 * b + c] += Mb * Tq[c];
    }
}

// res: shift S of the gradient modes (read when cbar is null); cbar: cotangent of the field (nel npt) or null; eslot: slot of every
// cell in ybuf (PS_DW); out: part (PS_VALUE, 3 doubles per block), the field (PS_FIELD), ybuf (PS_DW), d / d table (PS_DTABLE)
template <int NPC, int NVC, bool QUAD, bool UHAT, int MODE>
__global__ void __launch_bounds__(PLY_BLOCK)
k_ply_shear(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ shT, int npt, double rho,
            const double* __restrict__ w, const double* __restrict__ res, const double* __restrict__ cbar, const int* __restrict__ eslot,
            double* __restrict__ out) {
    constexpr int LD = 3 * NPC + 3 * NVC, NQ = QUAD ? 9 : 6;
    const int tid = threadIdx.x, e = blockIdx.x * PLY_BLOCK + tid;
    const bool live = e < m.nel && (MODE == PS_FIELD || cell_selected(m, e));
    double km = -INFINITY, kz = 0.0, area = 0.0;
    if (live) {
        Elem<NPC, NVC> el;
        load_elem<NPC, NVC, UHAT>(m, f, e, el);
        double ae = 0.0, gb0 = 0.0, gb1 = 0.0;
        {
            double xe[LD];
            load_state<NPC, NVC>(m, el, w, xe);
            for (int q = 0; q < NQ; ++q) {
                QPG g;
                qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, tab->N1[q], tab->dN1[q], g);
                double ga0, ga1;
                shear_q<NPC, NVC>(*tab, q, g, xe, ga0, ga1);
                const double wd = tab->w[q] * g.det, wj = wd * g.Ju;
                if constexpr (MODE == PS_VALUE) area += wd;  // alpha: area of the reference configuration, as for ply_failure
                ae += wj;
                gb0 += wj * ga0;
                gb1 += wj * ga1;
            }
        }
        const double ia = 1.0 / ae;
        gb0 *= ia;
        gb1 *= ia;
        if constexpr (MODE == PS_VALUE) {
            for (int p = 0; p < npt; ++p) {
                ShearPoint P;
                load_shear(shT, m.nel, e, p, P);
                const double t13 = P.G[0][0] * gb0 + P.G[0][1] * gb1, t23 = P.G[1][0] * gb0 + P.G[1][1] * gb1;
                ks_push_w(km, kz, rho * (P.F55 * t13 * t13 + P.F44 * t23 * t23), ae);
            }
        } else if constexpr (MODE == PS_FIELD) {
            for (int p = 0; p < npt; ++p) {
                ShearPoint P;
                load_shear(shT, m.nel, e, p, P);
                const double t13 = P.G[0][0] * gb0 + P.G[0][1] * gb1, t23 = P.G[1][0] * gb0 + P.G[1][1] * gb1;
                out[(size_t)e * npt + p] = P.F55 * t13 * t13 + P.F44 * t23 * t23;
            }
        } else {
            const double sh = cbar ? 0.0 : res[0];
            double d0 = 0.0, d1 = 0.0;                       // dK / dgbar (PS_DW)
            for (int p = 0; p < npt; ++p) {
                ShearPoint P;
                load_shear(shT, m.nel, e, p, P);
                const double t13 = P.G[0][0] * gb0 + P.G[0][1] * gb1, t23 = P.G[1][0] * gb0 + P.G[1][1] * gb1;
                const double c = cbar ? cbar[(size_t)e * npt + p] : ae * exp(rho * (P.F55 * t13 * t13 + P.F44 * t23 * t23) - sh);
                const double tb0 = 2.0 * c * P.F55 * t13, tb1 = 2.0 * c * P.F44 * t23;
                if constexpr (MODE == PS_DW) {
                    d0 += P.G[0][0] * tb0 + P.G[1][0] * tb1;
                    d1 += P.G[0][1] * tb0 + P.G[1][1] * tb1;
                } else {
                    double* o = out + ((size_t)e * npt + p) * PSH_W;
                    o[0] = tb0 * gb0; o[1] = tb0 * gb1; o[2] = tb1 * gb0; o[3] = tb1 * gb1;
                    o[4] = c * t13 * t13;
                    o[5] = c * t23 * t23;
                }
            }
            if constexpr (MODE == PS_DW) {
                d0 *= ia;
                d1 *= ia;
                double ye[LD];
#pragma unroll
                for (int i = 0; i < LD; ++i) ye[i] = 0.0;
                for (int q = 0; q < NQ; ++q) {
                    QPG g;
                    qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, tab->N1[q], tab->dN1[q], g);
                    const double wj = tab->w[q] * g.det * g.Ju;
                    shear_T_q<NPC, NVC>(*tab, q, g, wj * d0, wj * d1, ye);
                }
                double* dst = out + (size_t)eslot[e] * YSTRIDE;
#pragma unroll
                for (int i = 0; i < LD; ++i) dst[i] = ye[i];
            }
        }
    } else if (e < m.nel) {                      // outside the selected sub-domain
        if constexpr (MODE == PS_DW) ply_zero_ybuf_slot<LD>(eslot, e, out);
        else if constexpr (MODE == PS_DTABLE) ply_zero_table_row<PSH_W>(e, npt, out);
    }
    if constexpr (MODE == PS_VALUE) ply_block_slot(km, kz, area, tid, out);
}

}  // namespace femo
