// Forward mode of the field outputs: out[k] = (d field / d wrt) V[k] at the stored state and fields, gfx950, fp64.
//
// The reverse products of stress_grad.h and the aggregate's gradients of ply_failure.h run forwards.  A tangent needs no gather:
// every cell owns its entries of the output, so every kernel ends in plain stores and two identical calls return the same bits.
//
// DG1 von Mises fields ("stress", "stress_mid", "stress_bot"; c_e = M_e^-1 b_e, stress_grad.h):
//   dvm_q = d vm / d (e0, e1, g) . d(strain)_q,   db_i = sum_q w_q det_q N_i dvm_q,   dc_e = M_e^-1 db   (cell_mass_solve)
//   k_field_jvp       wrt w, h, E, nu: one thread per cell.  The directions loop INSIDE the loop over the quadrature points, FJ_ND to
//                     a pass: a point's geometry, frame, stress and d vm / d strain are formed once and serve every direction of the
//                     pass.  d(strain)_q is top_strain of the direction itself for w (the strains are linear in the state), the
//                     z = zf h and -zf b (x) gradx(dh) terms for h, dC/dE or dC/dnu for the material.  The db of the pass sit in the
//                     thread's own column of LDS (rolled direction loop, no barrier: columns are private).
//   k_field_jvp_uhat  wrt uhat: the dual arithmetic of shape_sens.h (field_uhat_db, the loop of k_field_uhat), the cell's nodal
//                     uhat carrying the direction as its dual part -- one thread per (direction, cell), one pass each.
// Zero stress: a point with vm_q = 0 contributes zero, as in the reverse products.
//
// Ply failure field (entry = max_q FI_eqp, k_ply_failure<PF_FIELD>):
//   k_ply_field_jvp   one thread per cell, one wave per block like the value kernel.  The state's six strains per point come through
//                     LDS into registers once; per direction the six tangent strains per point are formed once from dw_e and take the
//                     same road, and the recovery points stream through both.  Every point keeps (max FI, tangent at the max) with
//                     the value kernel's own update (a strict >, a NaN stays visible): on ties the first point in quadrature order
//                     wins.  TABLE: the direction is a table (entry-major like the table, through k_ply_transpose) and the tangent
//                     is d FI / d (G, z, F.) . dtable_ep at the maximiser.
#pragma once
#include "shell_device.h"
#include "shape_sens.h"
#include "stress.h"
#include "stress_grad.h"
#include "ply_failure.h"

namespace femo {

constexpr int FJ_ND = 4;           // directions that share one pass over the quadrature points
constexpr int FJ_BLOCK = 128;      // cells per block of k_field_jvp (FJ_ND * 4 columns of LDS: 16 KB)
enum { FJ_W = 1, FJ_H = 2, FJ_E = 3, FJ_NU = 4 };

// V: ndir directions of ldv entries (the state for FJ_W, else the nodal or per-cell field); out: ndir rows of ldo >= NVC nel entries
template <int NPC, int NVC, bool QUAD, bool UHAT>
__global__ void __launch_bounds__(FJ_BLOCK)
k_field_jvp(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ w, double zf, int mode, int ndir,
            const double* __restrict__ V, int64_t ldv, double* __restrict__ out, int64_t ldo) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    __shared__ double s_db[FJ_ND * NVC][FJ_BLOCK];
    const int tid = threadIdx.x, e = blockIdx.x * FJ_BLOCK + tid;
    if (e >= m.nel) return;
    Elem<NPC, NVC> el;
    load_elem<NPC, NVC, UHAT>(m, f, e, el);
    double xe[LD];
    load_state<NPC, NVC>(m, el, w, xe);
    const bool ewm = f.ewm != 0;
    const int nq = tab->nq;
    for (int k0 = 0; k0 < ndir; k0 += FJ_ND) {
        const int nk = min(FJ_ND, ndir - k0);
        for (int i = 0; i < nk * NVC; ++i) s_db[i][tid] = 0.0;
        for (int q = 0; q < nq; ++q) {
            QPG g;
            qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, tab->N1[q], tab->dN1[q], g);
            const double wd = tab->w[q] * g.det;
            const double hq = interp<NVC>(tab->N1[q], el.hn), Eq = interp<NVC>(tab->N1[q], el.En), nuq = interp<NVC>(tab->N1[q], el.nun);
            const TopStrain ts = top_strain<NPC, NVC>(*tab, q, g, el.hn, ewm, xe, hq, zf);
            double sig[3];
            const double vm = von_mises(ts, Eq, nuq, sig);
            if (!(vm > 0.0)) continue;                              // zero stress: zero contribution (subgradient)
            double de[3] = {0, 0, 0}, dvnu = 0.0;
            if (mode == FJ_W || mode == FJ_H) dvm_deps(sig, vm, Eq, nuq, de);
            if (mode == FJ_NU) {
                const double om = 1.0 - nuq * nuq, c = Eq / om, dc = 2.0 * nuq * Eq / (om * om);
                const double ds0 = dc * (ts.e0 + nuq * ts.e1) + c * ts.e1, ds1 = dc * (nuq * ts.e0 + ts.e1) + c * ts.e0;
                const double ds2 = dc * 0.5 * (1.0 - nuq) * ts.g - 0.5 * c * ts.g;
                dvnu = ((2.0 * sig[0] - sig[1]) * ds0 + (2.0 * sig[1] - sig[0]) * ds1 + 6.0 * sig[2] * ds2) / (2.0 * vm);
            }
#pragma unroll 1
            for (int kk = 0; kk < nk; ++kk) {
                const double* __restrict__ v = V + (size_t)(k0 + kk) * ldv;
                double dvm;
                if (mode == FJ_W) {
                    double dxe[LD];
                    load_state<NPC, NVC>(m, el, v, dxe);
                    const TopStrain dt = top_strain<NPC, NVC>(*tab, q, g, el.hn, ewm, dxe, hq, zf);      // linear in the state
                    dvm = de[0] * dt.e0 + de[1] * dt.e1 + de[2] * dt.g;
                } else if (mode == FJ_H) {
                    dvm = 0.0;
                    for (int b = 0; b < NVC; ++b) {
                        const double Mb = ewm ? 1.0 : tab->N1[q][b];
                        double d0 = -zf * Mb * ts.k00, d1 = -zf * Mb * ts.k11, d2 = -zf * Mb * ts.k01;
                        if (!ewm) {
                            const double r0 = tab->dN1[q][b][0], r1 = tab->dN1[q][b][1];
                            const double m0 = r0 * g.Q[0][0] + r1 * g.Q[1][0], m1 = r0 * g.Q[0][1] + r1 * g.Q[1][1];
                            d0 -= zf * ts.b0 * m0;
                            d1 -= zf * ts.b1 * m1;
                            d2 -= zf * (ts.b0 * m1 + ts.b1 * m0);
                        }
                        dvm += v[ewm ? e : el.vid[b]] * (de[0] * d0 + de[1] * d1 + de[2] * d2);
                        if (ewm) break;
                    }
                } else {
                    double dq = 0.0;                                // the direction interpolated as the field is
                    for (int b = 0; b < NVC; ++b) {
                        dq += v[ewm ? e : el.vid[b]] * (ewm ? 1.0 : tab->N1[q][b]);
                        if (ewm) break;
                    }
                    dvm = (mode == FJ_E ? vm / Eq : dvnu) * dq;
                }
                for (int i = 0; i < NVC; ++i) s_db[kk * NVC + i][tid] += wd * tab->N1[q][i] * dvm;
            }
        }
#pragma unroll 1
        for (int kk = 0; kk < nk; ++kk) {
            double db[NVC];
            for (int i = 0; i < NVC; ++i) db[i] = s_db[kk * NVC + i][tid];
            cell_mass_solve<NVC>(*tab, el.X, db);
            double* o = out + (size_t)(k0 + kk) * ldo + (size_t)NVC * e;
            for (int i = 0; i < NVC; ++i) o[i] = db[i];
        }
    }
}

// db_j = sum_q w_q det_q N_j d vm_q for the direction the nodal uhat carries as its dual part (det_q does not depend on uhat): the
// loop of k_field_uhat (stress_grad.h), which seeds one unit direction per thread and is left as it is
template <int NPC, int NVC, bool QUAD>
__device__ __forceinline__ void field_uhat_db(const Tables* __restrict__ tab, const Elem<NPC, NVC>& el, const D1 (*Uh)[3], const double* we,
                                              bool ewm, double zf, double* db) {
    for (int j = 0; j < NVC; ++j) db[j] = 0.0;
    const int nq = tab->nq;
    for (int q = 0; q < nq; ++q) {
        QPG g;
        double zero[NVC][3] = {};
        qp_geometry<NVC, QUAD, false>(el.X, zero, tab->N1[q], tab->dN1[q], g);
        QPD s;
        qp_shape_dual<NVC, QUAD>(el.X, Uh, tab->dN1[q], g, s);
        const double hq = interp<NVC>(tab->N1[q], el.hn), Eq = interp<NVC>(tab->N1[q], el.En), nuq = interp<NVC>(tab->N1[q], el.nun);
        const GenD sw = strains_dual<NPC, NVC>(*tab, q, g, s, we);
        double th[3] = {0, 0, 0};
        D1 gh0 = mk(0.0), gh1 = mk(0.0);
        for (int b = 0; b < NVC; ++b) {
            for (int c = 0; c < 3; ++c) th[c] += tab->NR[q][b] * we[3 * NPC + 3 * b + c];
            if (!ewm) {
                const double r0 = tab->dN1[q][b][0], r1 = tab->dN1[q][b][1];
                gh0 = gh0 + el.hn[b] * (r0 * s.Q[0][0] + r1 * s.Q[1][0]);
                gh1 = gh1 + el.hn[b] * (r0 * s.Q[0][1] + r1 * s.Q[1][1]);
            }
        }
        const double b0 = -dot3(th, g.E1), b1 = dot3(th, g.E0), z = zf * hq;
        const D1 e0 = sw.e00 - z * sw.k00 - (zf * b0) * gh0;
        const D1 e1 = sw.e11 - z * sw.k11 - (zf * b1) * gh1;
        const D1 gg = sw.g01 - z * sw.k01 - zf * (b0 * gh1 + b1 * gh0);
        const double cc = Eq / (1.0 - nuq * nuq);
        const D1 s0 = cc * (e0 + nuq * e1), s1 = cc * (nuq * e0 + e1), s2 = (cc * 0.5 * (1.0 - nuq)) * gg;
        const D1 vm = dsqrt(s0 * s0 - s0 * s1 + s1 * s1 + 3.0 * (s2 * s2));
        if (!(vm.v > 0.0)) continue;                                // zero stress: zero contribution (subgradient)
        const double wd = tab->w[q] * g.det;
        for (int j = 0; j < NVC; ++j) db[j] += wd * tab->N1[q][j] * vm.d;
    }
}

// V: ndir directions of 3 nn entries; one thread per (direction, cell)
template <int NPC, int NVC, bool QUAD>
__global__ void __launch_bounds__(128)
k_field_jvp_uhat(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ w, double zf, int ndir,
                 const double* __restrict__ V, int64_t ldv, double* __restrict__ out, int64_t ldo) {
    constexpr int LD = 3 * NPC + 3 * NVC;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)ndir * m.nel) return;
    const int k = (int)(gid / m.nel), e = (int)(gid - (int64_t)k * m.nel);
    const double* __restrict__ v = V + (size_t)k * ldv;
    Elem<NPC, NVC> el;
    load_elem<NPC, NVC, true>(m, f, e, el);
    D1 Uh[NVC][3];
    for (int b = 0; b < NVC; ++b)
        for (int i = 0; i < 3; ++i) Uh[b][i] = mk(el.Uh[b][i], v[3 * el.vid[b] + i]);
    double we[LD], db[NVC];
    load_state<NPC, NVC>(m, el, w, we);
    field_uhat_db<NPC, NVC, QUAD>(tab, el, Uh, we, f.ewm != 0, zf, db);
    cell_mass_solve<NVC>(*tab, el.X, db);
    double* o = out + (size_t)k * ldo + (size_t)NVC * e;
    for (int i = 0; i < NVC; ++i) o[i] = db[i];
}

// TABLE = false: V holds ndir state directions (ldv = ndof).  TABLE = true: V holds ndir table directions, entry-major like plyT
// (ldv = 16 npt nel).  out: ndir rows of ldo >= nel npt entries, out[k][e npt + p].
template <int NPC, int NVC, bool QUAD, bool UHAT, bool TABLE>
__global__ void __launch_bounds__(PLY_BLOCK)
k_ply_field_jvp(MeshDev m, FieldsDev f, const Tables* __restrict__ tab, const double* __restrict__ plyT, int npt, const double* __restrict__ w,
                int ndir, const double* __restrict__ V, int64_t ldv, double* __restrict__ out, int64_t ldo) {
    constexpr int LD = 3 * NPC + 3 * NVC, NQ = QUAD ? 9 : 6;
    __shared__ double s_q[6 * NQ][PLY_BLOCK];
    const int tid = threadIdx.x, e = blockIdx.x * PLY_BLOCK + tid;
    if (e >= m.nel) return;
    Elem<NPC, NVC> el;
    load_elem<NPC, NVC, UHAT>(m, f, e, el);
    // the six strains of every point of the state x, through the thread's column of LDS into registers
    auto point_strains = [&](const double* __restrict__ x, double (&s)[NQ][6]) {
        {
            double xe[LD];
            load_state<NPC, NVC>(m, el, x, xe);
            for (int q = 0; q < NQ; ++q) {
                QPG g;
                qp_geometry<NVC, QUAD, UHAT>(el.X, el.Uh, tab->N1[q], tab->dN1[q], g);
                const Gen sq = strains_q<NPC, NVC>(*tab, q, g, xe);
                s_q[6 * q + 0][tid] = sq.e00; s_q[6 * q + 1][tid] = sq.e11; s_q[6 * q + 2][tid] = sq.g01;
                s_q[6 * q + 3][tid] = sq.k00; s_q[6 * q + 4][tid] = sq.k11; s_q[6 * q + 5][tid] = sq.k01;
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int k = 0; k < 6; ++k) s[q][k] = s_q[6 * q + k][tid];
    };
    double s[NQ][6];
    point_strains(w, s);
    for (int k = 0; k < ndir; ++k) {
        const double* __restrict__ v = V + (size_t)k * ldv;
        double* o = out + (size_t)k * ldo + (size_t)e * npt;
        if constexpr (TABLE) {
            for (int p = 0; p < npt; ++p) {
                PlyPoint P, dP;
                load_ply(plyT, m.nel, e, p, P);
                load_ply(v, m.nel, e, p, dP);
                double mx = -INFINITY, dmx = 0.0;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double x[3], sig[3], sb[3], dsig[3];
                    const double fi = ply_fi(P, s[q], x, sig);
                    ply_dfi(P, sig, 1.0, sb);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        dsig[i] = 0.0;
#pragma unroll
                        for (int j = 0; j < 3; ++j) dsig[i] += dP.G[i][j] * x[j] - dP.z * P.G[i][j] * s[q][3 + j];
                    }
                    const double dfi = sb[0] * dsig[0] + sb[1] * dsig[1] + sb[2] * dsig[2] + dP.F1 * sig[0] + dP.F2 * sig[1] +
                                       dP.F11 * sig[0] * sig[0] + dP.F22 * sig[1] * sig[1] + dP.F66 * sig[2] * sig[2] +
                                       2.0 * dP.F12 * sig[0] * sig[1];
                    const bool take = fi > mx || fi != fi;          // the value kernel's update: a NaN stays visible
                    mx = take ? fi : mx;
                    dmx = take ? dfi : dmx;
                }
                o[p] = dmx;
            }
        } else {
            double ds[NQ][6];
            point_strains(v, ds);
            for (int p = 0; p < npt; ++p) {
                PlyPoint P;
                load_ply(plyT, m.nel, e, p, P);
                double mx = -INFINITY, dmx = 0.0;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double x[3], sig[3], sb[3], dx[3], dsig[3];
                    const double fi = ply_fi(P, s[q], x, sig);
                    ply_dfi(P, sig, 1.0, sb);
                    ply_fi(P, ds[q], dx, dsig);                     // sigma is linear in the strains: dsig = G (deps - z dkappa)
                    const double dfi = sb[0] * dsig[0] + sb[1] * dsig[1] + sb[2] * dsig[2];
                    const bool take = fi > mx || fi != fi;
                    mx = take ? fi : mx;
                    dmx = take ? dfi : dmx;
                }
                o[p] = dmx;
            }
        }
    }
}

}  // namespace femo
